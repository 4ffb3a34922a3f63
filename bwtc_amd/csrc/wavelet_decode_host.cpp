// Host half of the wavelet decoders 'B' / 'b' / 'u': record header, section lengths, tree shapes and the range
// decoder with its adaptive models (WaveletCoders.cpp:232-291, WaveletTree.hpp readShape :403-500, decodeTreeBF
// :857-1174, BitCoders.cpp:115-148, probmodels/ProbabilityModel.cpp:38-75), as bwtc_hip_decode.hpp states the
// format.  This part is serial by the format: a section's compressed length is not stored and the main model's
// state carries on from block to block.  What it leaves is a flattened forest (wavelet_rebuild.hpp): every node's
// bits go straight into one word array, a node's extent being known before its first bit is decoded.  Nothing
// here exits or throws on a corrupt record: every loop is bounded and every failure is a return code.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <new>

#include "wavelet_rebuild.hpp"

namespace bwtc_hip {

bool WrWordBuf::reserve(u64 words) {
  if (words <= cap) return true;
  u64 n = std::max<u64>(words + words / 2, 1u << 16);
  void* q = alloc ? alloc(n * 8) : std::malloc(n * 8);
  if (!q) return false;
  if (p) { std::memcpy(q, p, cap * 8); if (release) release(p); else std::free(p); }
  p = static_cast<u64*>(q);
  cap = n;
  return true;
}
void WrWordBuf::drop() {
  if (p) { if (release) release(p); else std::free(p); }
  p = nullptr; cap = 0;
}

namespace {

// MSB-first reader over the record; past its end it returns zeros and remembers
struct Bits {
  const u8* p; u64 n; u64 pos = 0; u32 bit = 0; bool over = false;
  u32 readBit() {
    if (pos >= n) { over = true; return 0; }
    const u32 b = (p[pos] >> (7 - bit)) & 1u;
    if (++bit == 8) { bit = 0; ++pos; }
    return b;
  }
  u64 readBits(u32 k) { u64 v = 0; while (k--) v = (v << 1) | readBit(); return v; }
  u32 readByte() {
    if (bit == 0) { if (pos >= n) { over = true; return 0; } return p[pos++]; }
    return (u32)readBits(8);
  }
  void flush() { if (bit) { bit = 0; ++pos; } }
  u64 packed() {                                                     // utils::readPackedInteger
    u64 result = 0, read = 0x80; u32 shift = 0;
    while ((read & 0x80) && shift < 64 && !over) { read = readBits(8); result |= (read & 0x7f) << shift; shift += 7; }
    return result;
  }
  u64 packedRev() {                                                  // utils::readPackedIntegerRev: bits of a byte LSB first
    u64 result = 0; u32 shift = 0, b;
    do {
      b = 0;
      for (int i = 0; i < 8; ++i) b |= readBit() << i;
      result |= (u64)(b & 0x7F) << shift;
      shift += 7;
    } while ((b & 0x80) && shift < 64 && !over);
    return result;
  }
};

u32 ceilLog2(u64 n) { u32 l = 0; while ((u64(1) << l) < n) ++l; return l; }
u64 binaryDecode(Bits& in, u64 lo, u64 hi) {                         // utils::binaryDecode
  const u64 range = hi - lo + 1;
  if (range == 1) return lo;
  const u32 k = ceilLog2(range);
  const u64 n_short = (u64(1) << k) - range, n_long_left = (range - n_short) / 2;
  u64 v = in.readBits(k - 1);
  if (v >= n_long_left) return v + lo;
  v = (v << 1) | in.readBit();
  return v < n_long_left ? v + lo : v + lo + n_short;
}
// utils::binaryInterpolativeDecode; false on a list that cannot be (a value outside its interval)
bool interpolativeDecode(Bits& in, std::vector<u32>& list, u64 lo, u64 hi, u64 elements) {
  if (elements == 0) return true;
  if (hi < lo || elements > hi - lo + 1) return false;
  if (elements == hi - lo + 1) { for (u64 v = lo; v <= hi; ++v) list.push_back((u32)v); return true; }
  const u64 h = (elements - 1) / 2, r = elements / 2 - h;
  const u64 mid = binaryDecode(in, lo + h, hi - h - r);
  if (in.over || mid < lo + h || mid > hi - h - r) return false;
  if (!interpolativeDecode(in, list, lo, mid - 1, h)) return false;
  list.push_back((u32)mid);
  return interpolativeDecode(in, list, mid + 1, hi, elements - h - 1);
}

// the three model sets as one table of fifteen predictors: main 0..7, gaps 8..11, integers 12..14
struct Models {
  char model;
  u32 q[15];
  u32 mc, gc, ic;
  explicit Models(char m) : model(m), mc(m == 'B' ? 4 : m == 'b' ? 3 : 0), gc(2), ic(1) { resetMain(); resetGaps(); resetInts(); }
  void resetMain() {                                                 // FSM8 keeps its state over a reset, FSM<N> does not
    static const u32 init[8] = {2400, 2300, 2200, 2100, 4096 - 2100, 4096 - 2200, 4096 - 2300, 4096 - 2400};
    for (int i = 0; i < 8; ++i) q[i] = model == 'B' ? init[i] : 2048;
    if (model == 'b') mc = 3;
  }
  void resetGaps() { for (int i = 8; i < 12; ++i) q[i] = 2048; gc = 2; }
  void resetInts() { for (int i = 12; i < 15; ++i) q[i] = 2048; ic = 1; }
  static u32 next(u32 states, u32 cur, bool bit) {
    if (states == 3) {
      if (cur == 1) return bit ? 2 : 0;
      if (cur == 2 && bit) return 2;
      if (cur == 0 && !bit) return 0;
      return 1;
    }
    if (bit) return cur >= states / 2 ? std::min(cur + 1, states - 1) : states / 2;
    return cur < states / 2 ? (cur ? cur - 1 : 0) : (states - 1) / 2;
  }
  void move(u32 slot, bool bit, u32 floor, u32 delay) {
    q[slot] = bit ? q[slot] + (((4096 - floor) - q[slot]) >> delay) : q[slot] - ((q[slot] - floor) >> delay);
  }
  void moveEven(u32 slot, bool bit) {
    if (bit) { if (q[slot] + 1024 < 4096) q[slot] += 1024; }
    else if (q[slot] > 1024) q[slot] -= 1024;
  }
  u32 mainP() const { return q[mc]; }
  void mainUpdate(bool bit) {
    if (model == 'B') move(mc, bit, 2, (mc == 0 || mc == 7) ? 4 : 5); else moveEven(mc, bit);
    mainState(bit);
  }
  void mainState(bool bit) { if (model == 'B') mc = next(8, mc, bit); else if (model == 'b') mc = next(6, mc, bit); }
  u32 gapP() const { return q[8 + gc]; }
  void gapUpdate(bool bit) { move(8 + gc, bit, 2, 5); gc = next(4, gc, bit); }
  u32 intP() const { return q[12 + ic]; }
  void intUpdate(bool bit) { move(12 + ic, bit, 100, 5); ic = next(3, ic, bit); }
};

struct RangeDecoder {                                                // BitDecoder
  u32 low, high, next;
  Bits* in;
  void start(Bits* r) {
    in = r; low = 0; high = 0xFFFFFFFFu; next = 0;
    for (int i = 0; i < 4; ++i) next = (next << 8) + in->readByte();
  }
  bool decode(u32 p1) {
    const u32 size = high - low - 1;
    const u32 split = low + (size >> 12) * p1 + (((size & 4095u) * p1 + 2048u) >> 12);
    const bool bit = next <= split;
    if (bit) high = split; else low = split + 1;
    while (((low ^ high) & 0xFF000000u) == 0) { low <<= 8; high = (high << 8) + 255; next = (next << 8) + in->readByte(); }
    return bit;
  }
};

struct GapBits {                                                     // gap vector of an inner node: host-only, read back in order
  std::vector<u64> w; u64 n = 0;
  void push(bool b) { if ((n & 63) == 0) w.push_back(0); w.back() |= (u64)b << (n & 63); ++n; }
  bool operator[](u64 i) const { return (w[i >> 6] >> (i & 63)) & 1; }
};

typedef std::pair<u64, u32> LenSym;

// one section's trees while they are decoded; links relative to the section
struct Section {
  std::vector<bwtc_hip_wforest_node> nodes;
  std::vector<bwtc_hip_wforest_code> codes;
  u32 symbolNodes = 0, W = 0;
  bool plainFixed = false;

  template <class N> static N blank() { N n; std::memset(&n, 0, sizeof(n)); n.left = n.right = -1; return n; }

  // WaveletTree::assignPrefixCodes; depth is bounded by the longest code, which readShape bounds
  template <class N>
  static size_t assign(std::vector<N>& pool, const std::vector<LenSym>& lengths, int nd, size_t elem, size_t depth) {
    if (elem >= lengths.size()) return elem;
    if (depth == lengths[elem].first - 1) {
      N leaf = blank<N>(); leaf.has_symbol = 1; leaf.symbol = lengths[elem].second;
      pool.push_back(leaf);
      const int c = (int)pool.size() - 1;
      if (pool[nd].left < 0) { pool[nd].left = c; return assign(pool, lengths, nd, elem + 1, depth); }
      pool[nd].right = c;
      return elem + 1;
    }
    if (pool[nd].left < 0) {
      pool.push_back(blank<N>());
      const int c = (int)pool.size() - 1;
      pool[nd].left = c;
      elem = assign(pool, lengths, c, elem, depth + 1);
    }
    if (elem < lengths.size()) {
      pool.push_back(blank<N>());
      const int c = (int)pool.size() - 1;
      pool[nd].right = c;
      elem = assign(pool, lengths, c, elem, depth + 1);
    }
    return elem;
  }

  // a set of code lengths that is no prefix code (Kraft sum above one) would make assign() drop symbols or hang
  // leaves below leaves; lengths sorted ascending
  static bool kraftOk(const std::vector<LenSym>& lengths, u64 maxLen) {
    long double sum = 0;
    for (const LenSym& l : lengths) { if (l.first == 0 || l.first > maxLen) return false; sum += std::ldexp(1.0L, -(int)l.first); }
    return sum <= 1.0L + 1e-12L;
  }

  int readShape(Bits& in) {
    nodes.assign(1, blank<bwtc_hip_wforest_node>());
    codes.assign(1, blank<bwtc_hip_wforest_code>());
    const u64 maxSym = in.readByte();
    u64 symbols = in.readByte();
    if (symbols == 0) symbols = 256;
    u64 maxLen = in.packedRev();
    if (in.over) return BWTC_HIP_E_PAST_RECORD;
    if (maxLen == 0 || maxLen > 255 || symbols > maxSym + 1) return BWTC_HIP_E_SHAPE;
    std::vector<u32> alphabet;
    if (!interpolativeDecode(in, alphabet, 0, maxSym, symbols)) return in.over ? BWTC_HIP_E_PAST_RECORD : BWTC_HIP_E_SHAPE;
    std::vector<LenSym> lengths;
    for (u64 i = 0; i < symbols; ++i) {
      u64 n = 1;
      while (!in.readBit()) { if (in.over) return BWTC_HIP_E_PAST_RECORD; if (++n > maxLen) return BWTC_HIP_E_SHAPE; }
      lengths.push_back(LenSym(maxLen - n + 1, alphabet[i]));
    }
    std::sort(lengths.begin(), lengths.end());
    if (!kraftOk(lengths, maxLen)) return BWTC_HIP_E_SHAPE;
    assign(nodes, lengths, 0, 0, 0);
    symbolNodes = (u32)nodes.size();
    const u64 longestRun = in.packedRev();
    if (in.over) return BWTC_HIP_E_PAST_RECORD;
    if (longestRun > 0xFFFFFFFFull) return BWTC_HIP_E_SHAPE;
    if (longestRun > 0) {
      symbols = in.packedRev();
      maxLen = in.packedRev();
      if (in.over) return BWTC_HIP_E_PAST_RECORD;
      if (symbols == 0 || symbols > longestRun + 1 || symbols > (1u << 22) || maxLen == 0 || maxLen > 4096) return BWTC_HIP_E_SHAPE;
      std::vector<u32> integers;
      if (!interpolativeDecode(in, integers, 0, longestRun, symbols)) return in.over ? BWTC_HIP_E_PAST_RECORD : BWTC_HIP_E_SHAPE;
      std::vector<LenSym> integerLengths;
      for (u64 i = 0; i < symbols; ++i) {
        u64 n = 1;
        while (!in.readBit()) { if (in.over) return BWTC_HIP_E_PAST_RECORD; if (++n > maxLen) return BWTC_HIP_E_SHAPE; }
        integerLengths.push_back(LenSym(maxLen + 1 - n, integers[i]));
      }
      std::sort(integerLengths.begin(), integerLengths.end());
      if (!kraftOk(integerLengths, maxLen)) return BWTC_HIP_E_SHAPE;
      assign(codes, integerLengths, 0, 0, 0);
    } else {
      codes[0].has_symbol = 1;                                       // the escape code is the empty word
      codes[0].symbol = 0;
      plainFixed = true;
    }
    W = (u32)in.readBits(4);
    return in.over ? BWTC_HIP_E_PAST_RECORD : 0;
  }
};

// writes one node's bits at the end of the word array
struct NodeWriter {
  u64* w; u64 n = 0;
  void push(bool b) { if ((n & 63) == 0) w[n >> 6] = 0; w[n >> 6] |= (u64)b << (n & 63); ++n; }
};

struct IntegerNode { int node, code; u64 bits; u32 leadingOnes; int status; };

}  // namespace

struct WDecoderState {
  Models models;
  Models prev;                       // the models before the last successful decode (wdecoder_undo)
  bool has_prev = false;
  explicit WDecoderState(char c) : models(c), prev(c) {}
};

WDecoderState* wdecoder_create(char coder) {
  if (coder != 'B' && coder != 'b' && coder != 'u') return nullptr;
  return new (std::nothrow) WDecoderState(coder);
}
void wdecoder_destroy(WDecoderState* d) { delete d; }
void wdecoder_reset(WDecoderState* d) { if (d) { d->models = Models(d->models.model); d->has_prev = false; } }
void wdecoder_undo(WDecoderState* d) { if (d && d->has_prev) { d->models = d->prev; d->has_prev = false; } }

namespace {

// decodeTreeBF: inner nodes breadth first, then the integer levels.  `budget` = words the forest may still take.
int decodeTree(Section& T, u64 rootSize, RangeDecoder& dec, Models& m, WrForest& F, u64 word_limit) {
  auto& nodes = T.nodes;
  auto begin = [&](int id, u64 bits, NodeWriter& wr) -> int {       // a node's extent is known before its first bit
    const u64 words = (bits + 63) / 64;
    if (F.n_words + words > word_limit) return BWTC_HIP_E_W_LIMIT;
    if (!F.words.reserve(F.n_words + words + 1)) return -2;
    nodes[id].bits = (u32)bits;
    nodes[id].first_word = (u32)F.n_words;
    wr.w = F.words.p + F.n_words; wr.n = 0;
    F.n_words += words;
    return 0;
  };
  typedef std::pair<int, GapBits> Inner;
  std::deque<Inner> queue;
  std::deque<IntegerNode> level;
  int rc;
  {
    GapBits left, right;
    NodeWriter wr;
    if ((rc = begin(0, rootSize, wr)) != 0) return rc;
    bool prev = dec.decode(m.mainP());
    m.mainUpdate(prev);
    wr.push(prev);
    (prev ? right : left).push(true);
    for (u64 i = 1; i < rootSize; ++i) {
      const bool bit = dec.decode(m.mainP());
      m.mainUpdate(bit);
      wr.push(bit);
      (bit ? right : left).push(prev != bit);
      prev = bit;
    }
    if (dec.in->over) return BWTC_HIP_E_PAST_RECORD;
    if (nodes[0].left < 0) return BWTC_HIP_E_SHAPE;
    if (left.n > 0) {
      if (nodes[nodes[0].left].has_symbol) level.push_back(IntegerNode{nodes[0].left, 0, left.n, 0, 0});
      else queue.push_back(Inner(nodes[0].left, std::move(left)));
    }
    if (right.n > 0) {
      if (nodes[0].right < 0) return BWTC_HIP_E_W_CHILD;
      if (nodes[nodes[0].right].has_symbol) level.push_back(IntegerNode{nodes[0].right, 0, right.n, 0, 0});
      else queue.push_back(Inner(nodes[0].right, std::move(right)));
    }
  }
  while (!queue.empty()) {
    m.resetMain();
    m.resetGaps();
    const int id = queue.front().first;
    GapBits gaps;
    std::swap(gaps, queue.front().second);
    queue.pop_front();
    if (nodes[id].left < 0 || nodes[id].right < 0) return BWTC_HIP_E_W_CHILD;
    const int l = nodes[id].left, r = nodes[id].right;
    GapBits left, right;
    NodeWriter wr;
    if ((rc = begin(id, gaps.n, wr)) != 0) return rc;
    bool prev = true;
    if (nodes[l].has_symbol && nodes[r].has_symbol) {
      u64 ones = 0;
      for (u64 i = 0; i < gaps.n; ++i) {
        if (!gaps[i]) prev = !prev;
        else { prev = dec.decode(m.gapP()); m.gapUpdate(prev); }
        wr.push(prev);
        ones += prev;
      }
      if (gaps.n > ones) level.push_back(IntegerNode{l, 0, gaps.n - ones, 0, 0});
      if (ones) level.push_back(IntegerNode{r, 0, ones, 0, 0});
    } else if (nodes[l].has_symbol) {
      for (u64 i = 0; i < gaps.n; ++i) {
        bool bit;
        if (!gaps[i] && !prev) bit = true;
        else if (gaps[i]) { bit = dec.decode(m.gapP()); m.gapUpdate(bit); m.mainState(bit); }
        else { bit = dec.decode(m.mainP()); m.mainUpdate(bit); }
        wr.push(bit);
        if (bit) right.push(prev != bit || gaps[i]);
        prev = bit;
      }
      if (gaps.n > right.n) level.push_back(IntegerNode{l, 0, gaps.n - right.n, 0, 0});
      if (right.n) queue.push_back(Inner(r, std::move(right)));
    } else if (!nodes[r].has_symbol) {
      for (u64 i = 0; i < gaps.n; ++i) {
        bool bit;
        if (gaps[i]) { bit = dec.decode(m.gapP()); m.gapUpdate(bit); m.mainState(bit); }
        else { bit = dec.decode(m.mainP()); m.mainUpdate(bit); }
        wr.push(bit);
        (bit ? right : left).push(prev != bit || gaps[i]);
        prev = bit;
      }
      if (left.n) queue.push_back(Inner(l, std::move(left)));
      if (right.n) queue.push_back(Inner(r, std::move(right)));
    } else {
      return BWTC_HIP_E_SHAPE;                                       // a shape the encoder cannot produce
    }
    if (dec.in->over) return BWTC_HIP_E_PAST_RECORD;
  }
  // integer levels: all nodes of a level, then its left children, then its right children
  auto child = [&](int nd, bool right) -> int {
    const int c = right ? nodes[nd].right : nodes[nd].left;
    if (c >= 0) return c;
    nodes.push_back(Section::blank<bwtc_hip_wforest_node>());
    const int id = (int)nodes.size() - 1;
    (right ? nodes[nd].right : nodes[nd].left) = id;
    return id;
  };
  std::deque<IntegerNode> lefts, rights;
  while (!level.empty()) {
    m.resetInts();
    lefts.clear(); rights.clear();
    while (!level.empty()) {
      IntegerNode nd = level.front();
      level.pop_front();
      if (nd.code >= 0 && T.codes[nd.code].has_symbol && T.codes[nd.code].symbol != 0) continue;
      NodeWriter wr;
      if ((rc = begin(nd.node, nd.bits, wr)) != 0) return rc;
      u64 ones = 0;
      for (u64 i = 0; i < nd.bits; ++i) {
        const bool bit = dec.decode(m.intP());
        m.intUpdate(bit);
        ones += bit;
        wr.push(bit);
      }
      if (dec.in->over) return BWTC_HIP_E_PAST_RECORD;
      const bool inCode = nd.code >= 0 && !T.codes[nd.code].has_symbol;
      if (nd.bits > ones) {
        IntegerNode c = {child(nd.node, false), inCode ? T.codes[nd.code].left : -1, nd.bits - ones, nd.leadingOnes, nd.status};
        if (inCode && c.code < 0) return BWTC_HIP_E_W_CHILD;
        if (c.code < 0) {
          if (nd.status == 0) { c.status = 2; c.leadingOnes = T.W; }
          else if (nd.status == 1) { c.status = 2; c.leadingOnes += T.W; }
          else --c.leadingOnes;
        }
        if (c.status != 2 || c.leadingOnes > 0) lefts.push_back(c);
      }
      if (ones > 0) {
        IntegerNode c = {child(nd.node, true), inCode ? T.codes[nd.code].right : -1, ones, nd.leadingOnes, nd.status};
        if (inCode && c.code < 0) return BWTC_HIP_E_W_CHILD;
        if (c.code < 0) {
          if (nd.status == 0) { c.status = 1; ++c.leadingOnes; }
          else if (nd.status == 1) ++c.leadingOnes;
          else --c.leadingOnes;
          if (c.status == 1 && c.leadingOnes > kWrMaxLeadingOnes) return BWTC_HIP_E_W_ESCAPE;
        }
        if (c.status != 2 || c.leadingOnes > 0) rights.push_back(c);
      }
    }
    level.insert(level.end(), lefts.begin(), lefts.end());
    level.insert(level.end(), rights.begin(), rights.end());
  }
  return 0;
}

int decodeRecord(Models& m, const u8* rec, u64 rec_bytes, u64 cap, WrForest& F, u64* consumed) {
  F.sections.clear(); F.nodes.clear(); F.codes.clear();
  F.n_words = 0; F.runs = 0; F.bytes = 0; F.n_lf = 0;
  if (rec_bytes < 6) return BWTC_HIP_E_PAST_RECORD;
  u64 compressed = 0;
  for (int i = 0; i < 6; ++i) compressed = (compressed << 8) | rec[i];
  const u64 rec_end = std::min<u64>(rec_bytes, 6 + compressed);
  const int past = rec_end < rec_bytes ? BWTC_HIP_E_LENGTH : BWTC_HIP_E_PAST_RECORD;
  Bits in{rec, rec_end};
  in.pos = 6;
  F.n_lf = in.readByte() + 1;
  for (u32 i = 0; i < F.n_lf; ++i) F.lf[i] = (u32)in.readBits(31);
  in.flush();
  u64 sections = in.readByte();
  if (sections == 0) sections = 256;
  u64 lengths[256], total = 0;
  for (u64 i = 0; i < sections; ++i) { lengths[i] = in.packed(); if (lengths[i] > cap) lengths[i] = cap + 1; total += lengths[i]; }
  if (in.over) return past;
  if (total > cap) return BWTC_HIP_E_CAPACITY;
  if (total >= (u64(1) << 31)) return BWTC_HIP_E_W_LIMIT;
  F.bytes = total;
  RangeDecoder dec;
  for (u64 s = 0; s < sections; ++s) {
    if (lengths[s] == 0) continue;
    const u64 rootSize = in.packed();
    if (in.over) return past;
    if (rootSize == 0 || rootSize > lengths[s]) return BWTC_HIP_E_W_TOTAL;
    Section T;
    int rc = T.readShape(in);
    if (rc) return rc == BWTC_HIP_E_PAST_RECORD ? past : rc;
    in.flush();
    dec.start(&in);
    // sanity bound of the forest's size: a product stream spends a few bits per run, far below 4 x 64 per byte
    const u64 word_limit = std::min<u64>(0xFFFFFFF0ull, 4 * total + F.nodes.size() + T.nodes.size() + (1u << 16));
    rc = decodeTree(T, rootSize, dec, m, F, word_limit);
    if (rc) return rc == BWTC_HIP_E_PAST_RECORD ? past : rc;
    if (in.over) return past;
    bwtc_hip_wforest_section S;
    S.runs = (u32)rootSize; S.bytes = (u32)lengths[s];
    S.first_node = (u32)F.nodes.size(); S.symbol_nodes = T.symbolNodes; S.n_nodes = (u32)T.nodes.size();
    S.first_code = (u32)F.codes.size(); S.n_codes = (u32)T.codes.size();
    S.W = T.W; S.plain_fixed = T.plainFixed ? 1u : 0u;
    if ((u64)F.nodes.size() + T.nodes.size() > 0x7FFFFFFFull || (u64)F.codes.size() + T.codes.size() > 0x7FFFFFFFull) return BWTC_HIP_E_W_LIMIT;
    F.sections.push_back(S);
    F.nodes.insert(F.nodes.end(), T.nodes.begin(), T.nodes.end());
    F.codes.insert(F.codes.end(), T.codes.begin(), T.codes.end());
    F.runs += rootSize;
    m.resetMain(); m.resetInts(); m.resetGaps();                    // endContextBlock
  }
  if (in.pos > rec_end || in.over) return past;
  if (in.pos - 6 != compressed) return BWTC_HIP_E_LENGTH;
  *consumed = in.pos;
  return 0;
}

}  // namespace

int wavelet_range_decode(WDecoderState& d, const u8* rec, u64 rec_bytes, u64 cap, WrForest& out, u64* consumed) {
  const Models before = d.models;
  int rc;
  try { rc = decodeRecord(d.models, rec, rec_bytes, cap, out, consumed); }
  catch (const std::bad_alloc&) { rc = -2; }
  if (rc) d.models = before;
  else { d.prev = before; d.has_prev = true; }
  return rc;
}

}  // namespace bwtc_hip
