// CPU-only test of the 'B' coder's model passes run lane by lane on the host (gm::modelsOnHostLanes,
// bwtc_amd/csrc/wavelet_gpu_models.hpp), meant for the sanitizers (scripts/sanitize_host.sh): `packed` and `out`
// live in heap buffers of exactly the sizes the device path allots -- whole 16-byte pieces, n_coded + 8 elements --
// so that a lane that reads or writes past them (the five-word tail load of laneMap, the margins of sbits and
// snaps inside modelsOnHostLanes) is reported here, where on the device it would read a neighbour silently.
// The shapes are a handful of those of tests/gmmodel.py; w is compared with a sequential loop below.
// Also: laneBracket called directly on a slot space whose chains start 256 positions before a slot-chunk border
// (walked exactly: a closed bracket), 257 before one (bracketed: open) and exactly at one.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../bwtc_amd/csrc/wavelet_gpu_models.hpp"

namespace gm = bwtc::wavelet::gm;
using gm::u32;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Shape {
  std::vector<unsigned char> codes;                       // bit | gap flag << 1 per element
  std::vector<gm::Task> tasks;
  void task(u32 type, const std::vector<unsigned char>& v) {
    const u32 b = (u32)codes.size();
    codes.insert(codes.end(), v.begin(), v.end());
    tasks.push_back(gm::Task{b, (u32)codes.size(), type, 0});
  }
};

static u32 g_seed = 12345;
static u32 rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static std::vector<unsigned char> pattern(const std::vector<unsigned char>& pat, size_t n) {
  std::vector<unsigned char> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = pat[i % pat.size()];
  return v;
}
static std::vector<unsigned char> noise(size_t n, bool flags) {
  std::vector<unsigned char> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (unsigned char)((rnd() & 1u) | (flags && rnd() % 3 == 0 ? 2u : 0u));
  return v;
}

// the sequential coder's models: one loop over the tasks in coding order
static void reference(const Shape& s, u32 state, std::vector<unsigned short>* w, u32* state_out) {
  w->assign(s.codes.size(), 0);
  u32 mc = state;
  for (const gm::Task& t : s.tasks) {
    u32 gc = 2, ic = 1, q[gm::kSlots];
    for (u32 k = 0; k < gm::kSlots; ++k) q[k] = gm::slotInit(k);
    for (u32 i = t.begin; i < t.end; ++i) {
      const u32 bit = s.codes[i] & 1u, flag = s.codes[i] >> 1;
      u32 k;
      if (t.type == gm::kTRoot) { k = mc; mc = gm::next8(mc, bit); }
      else if (t.type == gm::kTGaps) { k = 8 + gc; gc = gm::next4(gc, bit); }
      else if (t.type == gm::kTInts) { k = 12 + ic; ic = gm::next3(ic, bit); }
      else { k = flag ? 8 + gc : mc; mc = gm::next8(mc, bit); if (flag) gc = gm::next4(gc, bit); }
      const u32 x = q[k];
      q[k] = gm::moved(x, bit, gm::slotFloor(k), gm::slotDelay(k));
      (*w)[i] = (unsigned short)((bit << 15) | (bit ? x : 4096u - x));
    }
  }
  *state_out = mc;
}

static void run(const char* name, const Shape& s, u32 state, bool quiet = false) {
  const u32 n = (u32)s.codes.size();
  std::vector<gm::Task> tasks = s.tasks;
  std::vector<gm::Chunk> chunks;
  gm::cutChunks(&tasks, &chunks);
  const size_t words = ((size_t)n + 63) / 64 * 4;          // whole 16-byte pieces, as wavelet_models_prepare's input is
  std::unique_ptr<u32[]> packed(new u32[words]);
  std::memset(packed.get(), 0, words * 4);
  for (u32 i = 0; i < n; ++i) packed[i >> 4] |= (u32)s.codes[i] << ((i & 15u) * 2u);
  std::unique_ptr<unsigned short[]> out(new unsigned short[(size_t)n + 8]);   // reserve_models: n_coded + 8 elements
  u32 st = state;
  const bool ok = gm::modelsOnHostLanes(packed.get(), n, tasks, chunks, &st, out.get());
  CHECK(ok, "%s: the passes raised their error flag", name);
  std::vector<unsigned short> want;
  u32 want_state = 0;
  reference(s, state, &want, &want_state);
  u32 bad = n;
  for (u32 i = 0; i < n && bad == n; ++i) if (out[i] != want[i]) bad = i;
  CHECK(bad == n, "%s: w differs at element %u of %u (%u chunks)", name, bad, n, (u32)chunks.size());
  CHECK(st == want_state, "%s: state after the block %u, expected %u", name, st, want_state);
  if (!quiet || !ok || bad != n)
    std::printf("%-24s %7u elements %5u tasks %5u chunks  %s\n", name, n, (u32)tasks.size(), (u32)chunks.size(), ok && bad == n ? "ok" : "FAIL");
}

static void bracketBorders() {
  // slot 12 alone, four chains of zeros at 0, 1792, 3839 and 6144: 256 before the border 2048, 257 before 4096, at 6144
  const u32 nt = 4, ns = gm::kSlots * nt, starts[4] = {0, 1792, 3839, 6144}, total = 6144 + 2348;
  std::vector<u32> sb(ns + 1, 0);
  for (u32 k = 0; k < gm::kSlots; ++k)
    for (u32 t = 0; t < nt; ++t) sb[k * nt + t] = k < 12 ? 0 : k == 12 ? starts[t] : total;
  sb[ns] = total;
  std::unique_ptr<u32[]> sbits(new u32[total / 32 + 16]);
  std::memset(sbits.get(), 0, (total / 32 + 16) * 4);
  std::unique_ptr<gm::SlotMap[]> snaps(new gm::SlotMap[total / gm::kSample + 4]);
  const u32 floor = gm::slotFloor(12), d = gm::slotDelay(12);
  for (u32 j = 0; j < (total + gm::kSlotChunk - 1) / gm::kSlotChunk; ++j) {
    u32 err = 0;
    const gm::SlotMap m = gm::laneBracket(sbits.get(), sb.data(), ns, nt, total, j, snaps.get(), &err);
    CHECK(err == 0, "bracket %u: error %u", j, err);
    const gm::SlotMap at = snaps[j * gm::kSlotChunk / gm::kSample];
    if (j == 1 || j == 3) {
      u32 x = gm::slotInit(12);
      for (u32 i = 0; i < (j == 1 ? 256u : 0u); ++i) x = gm::moved(x, 0, floor, d);
      CHECK(at.mask == 0 && at.lo_x0 == x && (m.lo_x0 & 0xFFFFu) == x, "bracket %u: a chain %s the border is walked exactly: mask %x value %u, expected %u",
            j, j == 1 ? "256 positions before" : "at", at.mask, at.lo_x0, x);
    } else if (j == 2) {
      u32 lo = floor, hi = 4096u - floor;
      for (u32 i = 0; i < gm::kWarm; ++i) { lo = gm::moved(lo, 0, floor, d); hi = gm::moved(hi, 0, floor, d); }
      CHECK(hi > lo && at.mask == (1u << (hi - lo)) - 1u && at.lo_x0 == lo && (m.lo_x0 & 0xFFFFu) == lo,
            "bracket 2: a chain 257 positions before the border is bracketed: mask %x base %u, expected width %u base %u", at.mask, at.lo_x0, hi - lo, lo);
    }
  }
  std::printf("%-24s %s\n", "bracket borders", failures ? "FAIL" : "ok");
}

int main() {
  const u32 types[4] = {gm::kTRoot, gm::kTGaps, gm::kTInner, gm::kTInts};
  {
    Shape s;                                               // the tiny-task ladder: 1..5 elements, every bit pattern, every type
    for (u32 n = 1; n <= 5; ++n)
      for (u32 pat = 0; pat < (1u << n); ++pat)
        for (u32 ty = 0; ty < 4; ++ty) {
          std::vector<unsigned char> v(n);
          for (u32 i = 0; i < n; ++i) v[i] = (unsigned char)(((pat >> i) & 1u) | (rnd() % 3 == 0 ? 2u : 0u));
          s.task(types[ty], v);
        }
    for (u32 st = 0; st < 8; ++st) run("tiny ladder", s, st);
  }
  const size_t three = 3 * gm::kSlotChunk + 300;           // long enough for three slot-chunks in one slot
  {
    Shape s;
    s.task(gm::kTInts, pattern({1}, three));
    s.task(gm::kTInts, pattern({0}, three));
    run("constant integers", s, 3);
  }
  {
    Shape s;
    s.task(gm::kTInts, pattern({0, 1}, 3 * three));
    s.task(gm::kTInts, pattern({1, 0}, 3 * three + 1));
    run("alternating integers", s, 0);
  }
  {
    Shape s;
    s.task(gm::kTInts, pattern({0, 0, 1, 0, 1, 0}, 3 * three));
    s.task(gm::kTInts, pattern({0, 1, 1, 0, 1, 0, 0, 1}, 3 * three + 5));
    run("period-6 and -8 integers", s, 5);
  }
  {
    Shape s;                                               // chunks at every alignment: 67 elements each, types in turn
    for (u32 i = 0; i < 256; ++i) s.task(types[(i / 16) % 4], noise(67, true));
    run("every alignment", s, 6);
  }
  for (u32 n = 1; n <= 130; ++n) {                         // every length up to two pieces, ending the block: the tail loads' last words
    Shape s;
    s.task(types[n % 4], noise(n, true));
    s.task(gm::kTInts, pattern({0, 1}, n));
    s.task(gm::kTInner, noise(n, false));
    run("last words", s, n % 8, true);
  }
  {
    Shape s;                                               // a cell border inside a task, the chunk before it of 31..65 elements
    for (u32 n : {31u, 32u, 33u, 63u, 64u, 65u}) {
      const size_t border = (s.codes.size() + n + gm::kChunk - 1) / gm::kChunk * gm::kChunk;
      while (s.codes.size() + n < border) {
        const size_t room = border - n - s.codes.size(), m = 1 + rnd() % 64;
        s.task(types[rnd() % 4], noise(m < room ? m : room, true));
      }
      s.task(n & 1 ? gm::kTInner : gm::kTInts, noise(n + 100, false));
    }
    run("borders inside tasks", s, 2);
  }
  bracketBorders();
  if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
  std::printf("model lanes: all ok\n");
  return 0;
}
