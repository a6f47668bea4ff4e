// Host-only use of csrc/philox.h (no HIP, no GPU), built and run as a child process by tests/test_dare_cpu.py.
// Prints the three known answers of Philox4x32-10 as "kat w0 w1 w2 w3", then for every argument "i:m:stream:seed" (decimal)
// the draw of element i of source m as DARE defines it (include/vlm_hip.h, the DARE block, step 2) as "draw u".
#include "philox.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static void kat(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const philox4_t r = philox4x32_10(c0, c1, c2, c3, k0, k1);
  printf("kat %08x %08x %08x %08x\n", r.w[0], r.w[1], r.w[2], r.w[3]);
}

int main(int argc, char** argv) {
  kat(0, 0, 0, 0, 0, 0);
  kat(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
  kat(0x243f6a88u, 0x85a308d3u, 0x13198a2e, 0x03707344u, 0xa4093822u, 0x299f31d0u);
  for (int a = 1; a < argc; ++a) {
    unsigned long long v[4];
    char* p = argv[a];
    for (int k = 0; k < 4; ++k) {
      char* end = nullptr;
      v[k] = strtoull(p, &end, 10);
      if (end == p || (k < 3 ? *end != ':' : *end != '\0')) {
        fprintf(stderr, "bad argument %s\n", argv[a]);
        return 2;
      }
      p = end + 1;
    }
    if ((v[0] >> 2) >= (1ull << 32) || v[1] >= (1ull << 32) || v[2] >= (1ull << 32)) {
      fprintf(stderr, "out of range: %s\n", argv[a]);
      return 2;
    }
    const philox4_t r = dare_draw4(v[3], (uint32_t)v[2], (uint32_t)v[1], (uint32_t)(v[0] >> 2));
    printf("draw %u\n", r.w[v[0] & 3]);
  }
  return 0;
}
