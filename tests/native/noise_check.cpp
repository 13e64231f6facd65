// noise_check.cpp -- csrc/noise.h on the host (the same functions the kernels call), for tests/test_train_noise_host.py:
//   noise_check kat                                          the three Random123 known-answer vectors, one line of four hex words each
//   noise_check words <seed> <site> <sample> <draw> <n>      n words, one hex word per line
//   noise_check thr <rate>                                   dropout_threshold(rate)
// Built with g++ under -fsanitize=address,undefined by the test.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "noise.h"

using namespace hvla;

static void line(const PhiloxWords& w) { printf("%08x %08x %08x %08x\n", w.w[0], w.w[1], w.w[2], w.w[3]); }

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "kat")) {
    line(philox4x32_10(0, 0, 0, 0, 0, 0));
    line(philox4x32_10(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu));
    line(philox4x32_10(0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u));
    return 0;
  }
  if (argc == 7 && !strcmp(argv[1], "words")) {
    const unsigned long long seed = strtoull(argv[2], nullptr, 0);
    NoiseKey k;
    k.k0 = (uint32_t)seed; k.k1 = (uint32_t)(seed >> 32);
    k.site = (uint32_t)strtoul(argv[3], nullptr, 0);
    k.sample0 = strtol(argv[4], nullptr, 0);
    k.draw = (uint32_t)strtoul(argv[5], nullptr, 0);
    const long n = strtol(argv[6], nullptr, 0);
    for (long e = 0; e < n; ++e) printf("%08x\n", noise_block(k, 0, (uint32_t)(e >> 2)).w[e & 3]);
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "thr")) {
    printf("%u\n", dropout_threshold(strtof(argv[2], nullptr)));
    return 0;
  }
  fprintf(stderr, "usage: noise_check kat | words <seed> <site> <sample> <draw> <n> | thr <rate>\n");
  return 2;
}
