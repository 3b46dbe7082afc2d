// Stand-alone robustness check of the host JPEG entropy decoder (sdp-net_amd/csrc/jpeg_host.h), meant
// to be built for the CPU with -fsanitize=address,undefined and run on its own:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I sdp-net_amd/csrc tools/jpeg_host_check.cpp -o jpeg_host_check
//   ./jpeg_host_check a.jpg b.jpg
//
// For every file: the file itself must decode (code 0); then every prefix and every single-byte
// change (all 255 other values at every position) is probed and decoded.  Each variant lives in a
// heap block of exactly its length and the coefficients go into a heap block of exactly the
// capacity passed, so a read past `len` or a write past `coef_cap` is a sanitizer report.  A variant
// may decode, be unsupported or be malformed; what is checked is that every prefix is refused and
// that nothing reads or writes out of bounds or overflows.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "jpeg_host.h"

struct Tally {
  long ok = 0, unsupported = 0, malformed = 0;
  void add(int rc) { (rc == 0 ? ok : rc > 0 ? unsupported : malformed)++; }
};

static int run(const uint8_t* src, int64_t len, Tally& t, int64_t cap_override = -1) {
  uint8_t* data = (uint8_t*)malloc(len ? (size_t)len : 1);
  memcpy(data, src, (size_t)len);
  int32_t info[sdpjpeg::INFO_WORDS], info2[sdpjpeg::INFO_WORDS];
  const int prc = sdpjpeg::probe(data, len, info);
  int64_t cap = prc == 0 ? info[sdpjpeg::I_NCOEF] : 64;
  if (cap_override >= 0) cap = cap_override;
  int16_t* coef = (int16_t*)malloc(cap ? (size_t)cap * sizeof(int16_t) : 1);
  uint8_t qt[192];
  const int rc = sdpjpeg::entropy_decode(data, len, coef, cap, qt, info2);
  if (prc != 0 && rc != prc) {
    fprintf(stderr, "probe says %d, decode says %d (len %lld)\n", prc, rc, (long long)len);
    exit(2);
  }
  if (rc == 0 && memcmp(info, info2, sizeof(info)) != 0) {
    fprintf(stderr, "probe and decode disagree on info (len %lld)\n", (long long)len);
    exit(2);
  }
  t.add(rc);
  free(coef);
  free(data);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]);
    return 2;
  }
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      perror(argv[a]);
      return 2;
    }
    std::vector<uint8_t> buf;
    uint8_t chunk[4096];
    size_t n;
    while ((n = fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    fclose(f);
    const int64_t len = (int64_t)buf.size();
    Tally whole, prefixes, changes, caps;
    if (run(buf.data(), len, whole) != 0) {
      fprintf(stderr, "%s: the unmodified file does not decode\n", argv[a]);
      return 1;
    }
    for (int64_t k = 0; k < len; ++k)
      if (run(buf.data(), k, prefixes) >= 0) {
        fprintf(stderr, "%s: prefix of %lld bytes was not refused\n", argv[a], (long long)k);
        return 1;
      }
    std::vector<uint8_t> v(buf);
    for (int64_t k = 0; k < len; ++k) {
      for (int x = 1; x < 256; ++x) {
        v[k] = (uint8_t)(buf[k] ^ x);
        run(v.data(), len, changes);
      }
      v[k] = buf[k];
    }
    int32_t info[sdpjpeg::INFO_WORDS];
    sdpjpeg::probe(buf.data(), len, info);
    for (int64_t cap : {(int64_t)0, (int64_t)63, (int64_t)info[sdpjpeg::I_NCOEF] - 1})
      if (run(buf.data(), len, caps, cap) != sdpjpeg::ERR_CAPACITY) {
        fprintf(stderr, "%s: capacity %lld was not refused\n", argv[a], (long long)cap);
        return 1;
      }
    printf("%s: %lld bytes; prefixes refused %ld; single-byte changes: %ld decoded, %ld unsupported, %ld malformed\n",
           argv[a], (long long)len, prefixes.malformed, changes.ok, changes.unsupported, changes.malformed);
  }
  printf("clean\n");
  return 0;
}
