// Development: host cost of the 'B' coder's range-coder chains of one text block, three ways,
// with T threads doing the same at once (each on its own copy of the data), on synthetic
// w-streams (bit << 15 | probability of the coded bit) with the text block's section lengths
// divided by `scale`:
//   chain   the longest section alone in the scalar loop (runChainW)
//   lanes   the other 39 sections on a 16-lane engine (runCoderLanes): today's route is chain + lanes
//   fused   all of them through runChainsWithLanes (one vector step of the lanes per K long-chain elements)
//   full    the long chain with sixteen lanes kept busy all through it: the fused loop's cost per
//           long-chain element against `chain`'s
// Every chain's bytes are checked against runChainW.  One JSON line per measurement.
//   g++ -O2 -std=c++17 -Ibwtc_amd/csrc scripts/dev/chain_lanes_bench.cpp -Lbwtc_amd/lib -lbwtc_hip \
//       -Wl,-rpath,$PWD/bwtc_amd/lib -lpthread -o scripts/dev/bin/chain_lanes_bench
//   scripts/dev/bin/chain_lanes_bench <threads> <scale> <repeats>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "wavelet_rc.hpp"

using namespace bwtc::wavelet;
typedef std::chrono::steady_clock Clock;

namespace {

// the text block's sections (Mi coded elements): the longest, then the 39 others (the eleven
// largest as measured, the rest a geometric tail that brings them to 242 Mi)
std::vector<double> textSections() {
  std::vector<double> s = {265.6, 44.6, 38.9, 25.0, 21.8, 21.2, 20.6, 20.0, 11.3, 10.6, 5.9, 2.0};
  double left = 242.0 - 221.9, x = 1.9;
  for (int i = 0; i < 28; ++i) { const double v = i == 27 ? left : std::min(left, x); s.push_back(v); left -= v; x *= 0.86; }
  return s;
}

// a modelled stream: per element a model's confidence q, the bit drawn from it, the probability of
// the coded bit as the model says (about a byte per ten elements, as the text block's sections)
void makeW(std::vector<uint16_t>& w, uint64_t seed) {
  std::mt19937_64 rng(seed);
  for (size_t i = 0; i < w.size(); ++i) {
    const uint64_t r = rng();
    const double u = static_cast<double>(r & 0xFFFFF) / 1048576.0;
    const double q = 0.5 + 0.4995 * u;
    const bool likely = static_cast<double>((r >> 20) & 0xFFFFF) / 1048576.0 < q;
    uint32_t p = static_cast<uint32_t>((likely ? q : 1.0 - q) * 4096.0);
    p = std::max(1u, std::min(4095u, p));
    w[i] = static_cast<uint16_t>((likely ? 1u : 0u) << 15 | p);
  }
}

struct Chain { uint64_t begin, end; std::vector<uint8_t> out; };

struct Source : ChainSource {
  const uint16_t* w = nullptr;
  std::vector<Chain>* chains = nullptr;
  size_t at = 0;
  Source* other = nullptr;
  Clock::time_point last_done;
  bool next(ChainDesc* d) override {
    if (at >= chains->size()) return false;
    Chain& c = (*chains)[at++];
    c.out.clear();
    d->codes = nullptr; d->prob = nullptr; d->w = w;
    d->begin = c.begin; d->end = c.end; d->out = &c.out; d->cookie = &c;
    return true;
  }
  void done(void*) override { last_done = Clock::now(); }
  bool retire() override { return at >= chains->size() && (!other || other->at >= other->chains->size()); }
};

struct ThreadData {
  std::vector<uint16_t> w;
  std::vector<Chain> longs, shorts, full_shorts;
  std::vector<std::vector<uint8_t> > want_longs, want_shorts, want_full;
};

std::vector<std::vector<uint8_t> > reference(const std::vector<Chain>& cs, const uint16_t* w) {
  std::vector<std::vector<uint8_t> > r(cs.size());
  for (size_t i = 0; i < cs.size(); ++i) {
    CoderChain c;
    c.start(cs[i].begin, cs[i].end, &r[i]);
    runChainW(c, w, cs[i].end);
    c.finish();
  }
  return r;
}

bool same(const std::vector<Chain>& cs, const std::vector<std::vector<uint8_t> >& want) {
  for (size_t i = 0; i < cs.size(); ++i) if (cs[i].out != want[i]) return false;
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const int T = argc > 1 ? std::atoi(argv[1]) : 16;
  const double scale = argc > 2 ? std::atof(argv[2]) : 8.0;
  const int repeats = argc > 3 ? std::atoi(argv[3]) : 3;
  if (!simdCoderAvailable()) { std::printf("{\"error\": \"no AVX-512\"}\n"); return 1; }
  const std::vector<double> mi = textSections();
  std::vector<uint64_t> len(mi.size());
  uint64_t total = 0;
  for (size_t s = 0; s < mi.size(); ++s) { len[s] = static_cast<uint64_t>(mi[s] * 1048576.0 / scale); total += len[s]; }
  const uint64_t long_n = len[0], short_n = total - long_n;
  std::vector<ThreadData> td(T);
  {
    std::vector<std::thread> ts;
    for (int t = 0; t < T; ++t) ts.push_back(std::thread([&, t] {
      ThreadData& d = td[t];
      // the full-lanes case: sixteen chains as long as the long chain keeps sixteen lanes busy at K = 4, and more
      const uint64_t full_len = long_n / 4 + 4096;
      d.w.resize(total + 18 * full_len + 64);
      makeW(d.w, 1000 + t);
      uint64_t at = 0;
      for (size_t s = 0; s < len.size(); ++s) {
        Chain c; c.begin = at + (s * 7) % 16; c.end = at + len[s];
        (s == 0 ? d.longs : d.shorts).push_back(c);
        at += len[s];
      }
      for (int i = 0; i < 18; ++i) { Chain c; c.begin = at; c.end = at + full_len; d.full_shorts.push_back(c); at += full_len; }
      d.want_longs = reference(d.longs, d.w.data());
      d.want_shorts = reference(d.shorts, d.w.data());
      d.want_full = reference(d.full_shorts, d.w.data());
    }));
    for (size_t i = 0; i < ts.size(); ++i) ts[i].join();
  }
  uint64_t out_bytes = 0;
  for (size_t i = 0; i < td[0].want_longs.size(); ++i) out_bytes += td[0].want_longs[i].size();
  for (size_t i = 0; i < td[0].want_shorts.size(); ++i) out_bytes += td[0].want_shorts[i].size();
  std::printf("{\"threads\": %d, \"scale\": %.1f, \"long_elements\": %llu, \"short_elements\": %llu, \"sections\": %zu, \"bytes_per_element\": %.4f}\n",
              T, scale, (unsigned long long)long_n, (unsigned long long)short_n, len.size(), (double)out_bytes / total);
  std::fflush(stdout);

  // mode: 0 chain, 1 lanes, 2 fused (the block's mix), 3 full; returns per-thread seconds (and, for 2 and 3,
  // the seconds until the long chain was done in `long_s`)
  auto measure = [&](int mode, int K, std::vector<double>* secs, std::vector<double>* long_s) -> bool {
    std::atomic<int> ready{0};
    std::atomic<bool> go{false}, ok{true};
    secs->assign(T, 0.0);
    long_s->assign(T, 0.0);
    std::vector<std::thread> ts;
    for (int t = 0; t < T; ++t) ts.push_back(std::thread([&, t] {
      ThreadData& d = td[t];
      Source ls, ss;
      ls.w = ss.w = d.w.data();
      ls.chains = &d.longs;
      ss.chains = mode == 3 ? &d.full_shorts : &d.shorts;
      ls.other = &ss;
      ++ready;
      while (!go.load()) {}
      const auto t0 = Clock::now();
      if (mode == 0) {
        CoderChain c;
        d.longs[0].out.clear();
        c.start(d.longs[0].begin, d.longs[0].end, &d.longs[0].out);
        runChainW(c, d.w.data(), d.longs[0].end);
        c.finish();
      } else if (mode == 1) {
        runCoderLanes(ss, 16);
      } else {
        runChainsWithLanes(ls, ss, K);
      }
      const auto t1 = Clock::now();
      (*secs)[t] = std::chrono::duration<double>(t1 - t0).count();
      if (mode >= 2) (*long_s)[t] = std::chrono::duration<double>(ls.last_done - t0).count();
      if (!same(d.longs, d.want_longs) && mode != 1) ok = false;
      if (mode == 1 || mode == 2) { if (!same(d.shorts, d.want_shorts)) ok = false; }
      if (mode == 3 && !same(d.full_shorts, d.want_full)) ok = false;
    }));
    while (ready.load() < T) {}
    go = true;
    for (size_t i = 0; i < ts.size(); ++i) ts[i].join();
    return ok.load();
  };
  auto mean = [](const std::vector<double>& v) { double s = 0; for (size_t i = 0; i < v.size(); ++i) s += v[i]; return s / v.size(); };
  auto maxv = [](const std::vector<double>& v) { return *std::max_element(v.begin(), v.end()); };
  const int Ks[4] = {4, 5, 6, 8};
  std::vector<double> secs, lsecs;
  for (int r = 0; r < repeats; ++r) {
    bool ok = measure(0, 0, &secs, &lsecs);
    const double chain_ns = mean(secs) * 1e9 / long_n;
    std::printf("{\"repeat\": %d, \"mode\": \"chain\", \"ok\": %s, \"ns_per_long_element\": %.3f, \"core_s_per_block\": %.4f, \"max_thread_s\": %.4f}\n",
                r, ok ? "true" : "false", chain_ns, mean(secs) * scale, maxv(secs));
    ok = measure(1, 0, &secs, &lsecs);
    const double lanes_s = mean(secs);
    std::printf("{\"repeat\": %d, \"mode\": \"lanes\", \"ok\": %s, \"ns_per_short_element\": %.3f, \"core_s_per_block\": %.4f, \"chain_plus_lanes_core_s_per_block\": %.4f}\n",
                r, ok ? "true" : "false", lanes_s * 1e9 / short_n, lanes_s * scale, (chain_ns * long_n * 1e-9 + lanes_s) * scale);
    for (int q = 0; q < 4; ++q) {
      ok = measure(3, Ks[q], &secs, &lsecs);
      const double full_ns = mean(lsecs) * 1e9 / long_n;
      std::printf("{\"repeat\": %d, \"mode\": \"full\", \"K\": %d, \"ok\": %s, \"ns_per_long_element\": %.3f, \"vs_chain\": %.3f}\n",
                  r, Ks[q], ok ? "true" : "false", full_ns, full_ns / chain_ns);
      ok = measure(2, Ks[q], &secs, &lsecs);
      std::printf("{\"repeat\": %d, \"mode\": \"fused\", \"K\": %d, \"ok\": %s, \"core_s_per_block\": %.4f, \"long_done_s_per_block\": %.4f, \"max_thread_s_per_block\": %.4f}\n",
                  r, Ks[q], ok ? "true" : "false", mean(secs) * scale, mean(lsecs) * scale, maxv(secs) * scale);
      std::fflush(stdout);
    }
  }
  return 0;
}
