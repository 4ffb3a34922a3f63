// The range coder's long chains with the lanes stepped inside them (runChainsWithLanes,
// wavelet_rc.hpp) against each chain coded alone by runChainW: byte for byte, every chain, for
// every K, on uniform, skewed and extreme probabilities, chains of every length and alignment
// around the lane word, more lane chains than a long chain carries, sources that run dry and
// refill, long chains shorter than a lane's chain, no long chain at all, and several engines on
// the same sources; and the same lane chains through runCoderLanes (the other route's engine,
// one and two vectors).  Prints "ok" and exits 0 when all agree.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

#include "wavelet_rc.hpp"

using namespace bwtc::wavelet;

namespace {

std::vector<uint16_t> makeW(std::mt19937_64& rng, size_t n, int kind) {
  std::vector<uint16_t> w(n + 32);
  for (size_t i = 0; i < w.size(); ++i) {
    const uint64_t r = rng();
    uint32_t p;
    if (kind == 0) p = 1 + static_cast<uint32_t>(r % 4095);                                   // uniform
    else if (kind == 1) {                                                                       // skewed: mostly near-certain bits
      const double u = static_cast<double>(r >> 11) / 9007199254740992.0;
      p = 4095 - static_cast<uint32_t>(4094.0 * u * u * u * u);
    } else {                                                                                    // extreme
      static const uint32_t e[4] = {1, 2, 4094, 4095};
      p = e[r & 3];
    }
    const uint32_t bit = static_cast<uint32_t>(r >> 40) & 1u;
    w[i] = static_cast<uint16_t>(bit << 15 | p);
  }
  return w;
}

struct Chain {
  uint64_t begin, end;
  std::vector<uint8_t> out, want;
  size_t prefix;
};

// hands out its chains in order; `dry_every` > 0: every that many chains it answers "none" once
// before it goes on (the engines must come back for the rest)
struct Source : ChainSource {
  const uint16_t* w;
  std::vector<Chain>* chains;
  size_t at = 0, handed_since_dry = 0, dry_every = 0;
  std::atomic<size_t> finished{0};
  std::mutex* mu;                      // shared by the two sources of one run
  Source* other = nullptr;
  bool next(ChainDesc* d) override {
    std::lock_guard<std::mutex> g(*mu);
    if (at >= chains->size()) return false;
    if (dry_every && handed_since_dry == dry_every) { handed_since_dry = 0; return false; }
    ++handed_since_dry;
    Chain& c = (*chains)[at++];
    d->codes = nullptr; d->prob = nullptr; d->w = w;
    d->begin = c.begin; d->end = c.end; d->out = &c.out; d->cookie = &c;
    return true;
  }
  void done(void*) override { ++finished; }
  bool retire() override {
    std::lock_guard<std::mutex> g(*mu);
    return at >= chains->size() && (!other || other->at >= other->chains->size());
  }
};

int failures = 0;

void expectAll(const char* what, std::vector<Chain>& cs, size_t finished) {
  if (finished != cs.size()) { std::printf("FAIL %s: %zu of %zu chains finished\n", what, finished, cs.size()); ++failures; return; }
  for (size_t i = 0; i < cs.size(); ++i)
    if (cs[i].out != cs[i].want) {
      std::printf("FAIL %s: chain %zu [%llu, %llu) differs (%zu bytes, want %zu)\n", what, i,
                  (unsigned long long)cs[i].begin, (unsigned long long)cs[i].end, cs[i].out.size(), cs[i].want.size());
      ++failures;
      return;
    }
}

void prepare(std::vector<Chain>& cs, const uint16_t* w, std::mt19937_64& rng) {
  for (size_t i = 0; i < cs.size(); ++i) {
    Chain& c = cs[i];
    c.prefix = rng() % 5;
    c.out.assign(c.prefix, static_cast<uint8_t>(0xA5));            // a section's prefix
    c.want = c.out;
    CoderChain r;
    r.start(c.begin, c.end, &c.want);
    runChainW(r, w, c.end);
    r.finish();
  }
}

// longs / shorts: (length, begin) of each chain; threads engines at once
void run(const char* what, int kind, int k, const std::vector<std::pair<uint64_t, uint64_t> >& longs,
         const std::vector<std::pair<uint64_t, uint64_t> >& shorts, size_t dry_every, int threads, uint64_t seed) {
  std::mt19937_64 rng(seed);
  uint64_t n = 0;
  for (size_t i = 0; i < longs.size(); ++i) n = std::max(n, longs[i].second + longs[i].first);
  for (size_t i = 0; i < shorts.size(); ++i) n = std::max(n, shorts[i].second + shorts[i].first);
  const std::vector<uint16_t> w = makeW(rng, n, kind);
  std::vector<Chain> lc(longs.size()), sc(shorts.size());
  for (size_t i = 0; i < longs.size(); ++i) { lc[i].begin = longs[i].second; lc[i].end = longs[i].second + longs[i].first; }
  for (size_t i = 0; i < shorts.size(); ++i) { sc[i].begin = shorts[i].second; sc[i].end = shorts[i].second + shorts[i].first; }
  prepare(lc, w.data(), rng);
  prepare(sc, w.data(), rng);
  std::mutex mu;
  Source ls, ss;
  ls.w = ss.w = w.data();
  ls.chains = &lc; ss.chains = &sc;
  ls.mu = ss.mu = &mu;
  ls.other = &ss;
  ss.dry_every = dry_every;
  std::vector<std::thread> ts;
  for (int t = 0; t < threads; ++t) ts.push_back(std::thread([&] { runChainsWithLanes(ls, ss, k); }));
  for (size_t t = 0; t < ts.size(); ++t) ts[t].join();
  char name[160];
  std::snprintf(name, sizeof name, "%s (kind %d, K %d, long)", what, kind, k);
  expectAll(name, lc, ls.finished.load());
  std::snprintf(name, sizeof name, "%s (kind %d, K %d, lanes)", what, kind, k);
  expectAll(name, sc, ss.finished.load());
  // the same lane chains through the lane engine of the other route (runCoderLanes), one and two vectors
  for (int lanes = 16; lanes <= 32; lanes += 16) {
    std::vector<Chain> again(sc);
    for (size_t i = 0; i < again.size(); ++i) again[i].out.assign(sc[i].want.begin(), sc[i].want.begin() + sc[i].prefix);
    Source as;
    as.w = w.data(); as.chains = &again; as.mu = &mu; as.dry_every = dry_every;
    runCoderLanes(as, lanes);
    std::snprintf(name, sizeof name, "%s (kind %d, runCoderLanes %d)", what, kind, lanes);
    expectAll(name, again, as.finished.load());
  }
}

}  // namespace

int main() {
  if (!simdCoderAvailable()) { std::printf("skip: no AVX-512\n"); return 0; }
  std::mt19937_64 rng(11);
  typedef std::vector<std::pair<uint64_t, uint64_t> > List;
  const int ks[4] = {4, 5, 6, 8};
  for (int kind = 0; kind < 3; ++kind)
    for (int q = 0; q < 4; ++q) {
      // one long chain, forty lane chains of mixed lengths at mixed offsets
      List longs(1, std::make_pair(300000 + rng() % 1000, rng() % 16)), shorts;
      for (int i = 0; i < 40; ++i) shorts.push_back(std::make_pair(rng() % 60000, rng() % 100000));
      run("mixed", kind, ks[q], longs, shorts, 0, 1, 100 + q);
    }
  for (int q = 0; q < 4; ++q) {
    // chains shorter than a word, and just above the lanes' floor, at every alignment
    List longs(1, std::make_pair(200000, 3)), shorts;
    for (uint64_t off = 0; off < 16; ++off) {
      for (uint64_t len = 0; len < 40; ++len) shorts.push_back(std::make_pair(len, 1000 + off));
      for (uint64_t len = 510; len < 530; ++len) shorts.push_back(std::make_pair(len, 5000 + off));
    }
    run("short and unaligned", 1, ks[q], longs, shorts, 0, 1, 200 + q);
  }
  for (int q = 0; q < 4; ++q) {
    // more lane chains than the long chain carries: they drain after it, as a plain lane engine
    List longs(1, std::make_pair(10000, 0)), shorts;
    for (int i = 0; i < 100; ++i) shorts.push_back(std::make_pair(50000 + rng() % 100, rng() % 1000));
    run("lanes outlast the long chain", 0, ks[q], longs, shorts, 0, 1, 300 + q);
    // a long chain shorter than one lane's chain
    List longs2(1, std::make_pair(2000 + q, 5)), shorts2(3, std::make_pair(200000, 17));
    run("long chain shorter than a lane", 2, ks[q], longs2, shorts2, 0, 1, 400 + q);
    // the lanes' source runs dry every few chains and refills
    List longs3(2, std::make_pair(150000, 1)), shorts3;
    for (int i = 0; i < 60; ++i) shorts3.push_back(std::make_pair(1000 + rng() % 20000, rng() % 64));
    run("source runs dry and refills", 1, ks[q], longs3, shorts3, 5, 1, 500 + q);
  }
  {
    // no long chain at all; several long chains one after the other; several engines on shared sources
    List none, shorts;
    for (int i = 0; i < 50; ++i) shorts.push_back(std::make_pair(rng() % 30000, rng() % 300));
    run("no long chain", 0, 6, none, shorts, 0, 1, 600);
    List longs;
    for (int i = 0; i < 5; ++i) longs.push_back(std::make_pair(40000 + rng() % 40000, rng() % 100));
    run("several long chains", 1, 6, longs, shorts, 3, 1, 601);
    List longs4;
    for (int i = 0; i < 12; ++i) longs4.push_back(std::make_pair(100000 + rng() % 100000, rng() % 100));
    List shorts4;
    for (int i = 0; i < 300; ++i) shorts4.push_back(std::make_pair(rng() % 40000, rng() % 1000));
    run("four engines", 1, 6, longs4, shorts4, 7, 4, 602);
    run("long chains only", 2, 4, longs4, List(), 0, 3, 603);
  }
  if (failures) { std::printf("%d failures\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
