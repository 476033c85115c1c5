// bslz4_host_check — the host bitshuffle/LZ4 decoder under AddressSanitizer and
// UndefinedBehaviorSanitizer, stand-alone: the library's sources compiled with
// the sanitizers on the host side and linked into this program, which decodes
// every chunk of the conformance corpus (directed, malformed and mutated;
// tests/bslz4_ref.py --dump) into a heap buffer of exactly the stated size.
// It needs no GPU and is never loaded into Python.  From the repository root:
//
//   mkdir -p build && python tests/bslz4_ref.py --dump build/bslz4_corpus.bin && /opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fno-slp-vectorize -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -Iinclude -DBLDP_BUILD -x hip tools/bslz4_host_check.cpp bldistributeddataproducts.jl_amd/csrc/*.hip -ldl -o build/bslz4_host_check && build/bslz4_host_check build/bslz4_corpus.bin
//
// Corpus file (little-endian): "BSLZ4COR", uint32 count, then per chunk
// uint32 element size, uint32 verdict (1 = decodes), uint64 chunk bytes,
// uint64 expected bytes, the chunk, the expected bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bldp.h"

namespace {

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s CORPUS\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  char magic[8];
  uint32_t count = 0;
  if (!read_exact(f, magic, 8) || memcmp(magic, "BSLZ4COR", 8) || !read_exact(f, &count, 4)) {
    fprintf(stderr, "%s: not a corpus file\n", argv[1]);
    return 2;
  }
  unsigned calls = 0, accepted = 0, rejected = 0, failures = 0;
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t es = 0, verdict = 0;
    uint64_t clen = 0, wlen = 0;
    if (!read_exact(f, &es, 4) || !read_exact(f, &verdict, 4) || !read_exact(f, &clen, 8) ||
        !read_exact(f, &wlen, 8) || clen > (1u << 26) || wlen > (1u << 26)) {
      fprintf(stderr, "chunk %u: truncated record\n", k);
      return 2;
    }
    // heap copies of exactly the stated sizes: one byte past either is a report
    uint8_t *chunk = (uint8_t *)malloc(clen ? clen : 1);
    std::vector<uint8_t> want(wlen);
    if (!read_exact(f, chunk, clen) || !read_exact(f, want.data(), wlen)) {
      fprintf(stderr, "chunk %u: truncated record\n", k);
      return 2;
    }
    uint64_t nb = 0;
    uint32_t bb = 0;
    int rc = bldp_bslz4_info(chunk, clen, &nb, &bb);
    ++calls;
    if (rc != BLDP_OK || nb > (1u << 26)) {
      fprintf(stderr, "chunk %u: bldp_bslz4_info gives %d, %llu bytes\n", k, rc,
              (unsigned long long)nb);
      ++failures;
      free(chunk);
      continue;
    }
    uint8_t *out = (uint8_t *)malloc(nb ? nb : 1);
    rc = bldp_bslz4_decode_host(chunk, clen, (int)es, nb ? out : nullptr, nb);
    ++calls;
    if (verdict) {
      ++accepted;
      if (rc != BLDP_OK || nb != wlen || (wlen && memcmp(out, want.data(), wlen))) {
        fprintf(stderr, "chunk %u (es %u): expected to decode, rc %d\n", k, es, rc);
        ++failures;
      }
    } else {
      ++rejected;
      if (rc != BLDP_EINVAL) {
        fprintf(stderr, "chunk %u (es %u): expected BLDP_EINVAL, rc %d\n", k, es, rc);
        ++failures;
      }
    }
    free(out);
    free(chunk);
  }
  fclose(f);
  printf("%u chunks, %u calls: %u decoded, %u refused, %u failures\n", count, calls, accepted,
         rejected, failures);
  return failures ? 1 : 0;
}
