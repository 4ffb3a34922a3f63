// CPU-only check of the library's host half of the wavelet decoders (range decoder into a flattened forest + the
// host twin of the rebuild kernels) against the host mirror's WaveletDecoder and the oracle's transform: 'B', 'b'
// and 'u' streams of the oracle, one block and several blocks through ONE decoder handle (the main model's state
// crosses block borders).  No device call is made.
// TEST INFRASTRUCTURE: links the oracle (liboracle.so) as encoder and checker.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "bwtc_hip.hpp"
#include "bwtc_hip_decode.hpp"
#include "../../oracle/bwtc_oracle.h"

using namespace bwtc;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static void stream(char letter, const std::vector<byte>& data, size_t bs, uint32 sp, const char* what) {
  std::vector<byte> whole(orc_compress_bound(data.size()) + 8192 * (data.size() / bs + 2) + 100000);
  const size_t sn = orc_compress_wavelet(letter, &data[0], data.size(), bs, sp, &whole[0], whole.size());
  CHECK(sn > 0 && whole[0] == (byte)letter, "%s: oracle stream", what);
  MemoryBitReader in(&whole[0], sn);
  in.readByte();
  WaveletDecoder mirror(letter);
  bwtc_hip_wavelet_decoder* handle = bwtc_hip_wavelet_decoder_create(letter);
  CHECK(handle != 0, "%s: decoder handle", what);
  size_t off = 0;
  for (;;) {
    const uint64 n = in.readPackedInteger();
    if (n == 0) break;
    CHECK(in.readPackedInteger() == 1 && in.readByte() == 0, "%s: block prefix", what);
    std::vector<byte> t(data.begin() + off, data.begin() + off + n);
    t.push_back(0);
    std::vector<uint32> lf(256);
    uint32 n_lf = 0, freqs[256];
    std::memset(freqs, 0, sizeof freqs);
    orc_bwt_block(&t[0], (uint32)n, sp, &lf[0], &n_lf, freqs);
    // the library: a record may be followed by more bytes (the rest of the stream is)
    std::vector<byte> got(n + 16, 0xA5);
    uint32 glf[256], gn = 0, gsize = 0;
    uint64_t used = 0;
    const int rc = bwtc_hip_wavelet_decode_bwt_host(handle, in.here(), in.left(), &got[0], n, glf, &gn, &gsize, &used);
    CHECK(rc == 0, "%s: bwtc_hip_wavelet_decode_bwt_host returned %d at %zu", what, rc, off);
    CHECK(gsize == n && std::memcmp(&got[0], &t[0], n) == 0, "%s: library bytes differ from the oracle's BWT, block at %zu", what, off);
    CHECK(got[n] == 0xA5, "%s: byte past the block written", what);
    CHECK(gn == n_lf && std::memcmp(glf, &lf[0], n_lf * 4) == 0, "%s: library LF powers, block at %zu", what, off);
    // the host mirror's decoder over the same record
    const size_t before = in.position();
    std::vector<byte> out(n + 16);
    BWTBlock block(&out[0], 0, true);
    mirror.decodeBlock(block, in, n);
    CHECK(block.size() == gsize && std::memcmp(&out[0], &got[0], n) == 0, "%s: library differs from WaveletDecoder, block at %zu", what, off);
    CHECK(in.position() - before == used, "%s: consumed %llu, WaveletDecoder %zu", what, (unsigned long long)used, in.position() - before);
    off += n;
  }
  CHECK(off == data.size(), "%s: stream length", what);
  bwtc_hip_wavelet_decoder_destroy(handle);
}

int main() {
  std::mt19937 rng(777);
  std::vector<std::vector<byte> > inputs;
  const char* golden = "abracadabra";
  inputs.push_back(std::vector<byte>(golden, golden + 11));
  inputs.push_back(std::vector<byte>(1, 'x'));
  inputs.push_back(std::vector<byte>(30000, 65));
  { std::vector<byte> d(120000); for (size_t i = 0; i < d.size(); ++i) d[i] = (byte)rng(); inputs.push_back(d); }
  { std::vector<byte> d(90000); for (size_t i = 0; i < d.size(); ++i) d[i] = (byte)("ACGT"[rng() & 3]); inputs.push_back(d); }
  { std::vector<byte> d; while (d.size() < 400000) d.insert(d.end(), 1 + rng() % 3000, (byte)(rng() % 6)); inputs.push_back(d); }
  { std::vector<byte> seed(5000), d; for (size_t i = 0; i < seed.size(); ++i) seed[i] = (byte)(rng() % 40 + 60);
    while (d.size() < 300000) d.insert(d.end(), seed.begin(), seed.end());
    inputs.push_back(d); }
  { std::vector<byte> d(150000); for (size_t i = 0; i < d.size(); ++i) { unsigned v = 0; while ((rng() & 3) && v < 250) ++v; d[i] = (byte)v; } inputs.push_back(d); }
  char what[96];
  for (const char* letter = "Bbu"; *letter; ++letter)
    for (size_t k = 0; k < inputs.size(); ++k) {
      std::snprintf(what, sizeof what, "coder '%c' input %zu one block", *letter, k);
      stream(*letter, inputs[k], inputs[k].size(), 8, what);
      std::snprintf(what, sizeof what, "coder '%c' input %zu three blocks", *letter, k);
      stream(*letter, inputs[k], inputs[k].size() / 3 + 1, 4, what);
    }
  { std::vector<byte> data;
    for (int r = 0; r < 6; ++r) data.insert(data.end(), inputs[6].begin(), inputs[6].end());
    stream('B', data, 170000, 4, "coder 'B' eleven blocks"); }
  // a cut record and a flipped byte end in a return code
  { std::vector<byte> whole(orc_compress_bound(inputs[3].size()) + 100000);
    const size_t sn = orc_compress_wavelet('B', &inputs[3][0], inputs[3].size(), inputs[3].size(), 8, &whole[0], whole.size());
    const size_t head = 1 + 3 + 1 + 1;                                   // letter, packed 120000, slices, grammar
    std::vector<byte> out(inputs[3].size() + 16);
    uint32 glf[256], gn = 0, gsize = 0; uint64_t used = 0;
    bwtc_hip_wavelet_decoder* h = bwtc_hip_wavelet_decoder_create('B');
    CHECK(bwtc_hip_wavelet_decode_bwt_host(h, &whole[head], (sn - head) / 2, &out[0], inputs[3].size(), glf, &gn, &gsize, &used) == BWTC_HIP_E_PAST_RECORD,
          "a record cut in half");
    CHECK(bwtc_hip_wavelet_decode_bwt_host(h, &whole[head], sn - head, &out[0], inputs[3].size() - 1, glf, &gn, &gsize, &used) == BWTC_HIP_E_CAPACITY,
          "a block larger than the capacity");
    for (size_t at = head + 40; at < sn - 1; at += (sn - head) / 23) {
      std::vector<byte> bad(whole.begin(), whole.begin() + sn);
      bad[at] ^= 0x55;
      const int rc = bwtc_hip_wavelet_decode_bwt_host(h, &bad[head], sn - head, &out[0], inputs[3].size(), glf, &gn, &gsize, &used);
      CHECK(rc <= 0, "a flipped byte at %zu", at);                         // refused, or decoded to something of the right size
    }
    // the handle is as it was: the intact record still decodes
    CHECK(bwtc_hip_wavelet_decode_bwt_host(h, &whole[head], sn - head, &out[0], inputs[3].size(), glf, &gn, &gsize, &used) == 0 &&
          gsize == inputs[3].size(), "decode after refused records");
    bwtc_hip_wavelet_decoder_destroy(h); }
  std::printf(failures ? "%d FAILURES\n" : "wavelet rebuild (host): all tests passed\n", failures);
  return failures ? 1 : 0;
}
