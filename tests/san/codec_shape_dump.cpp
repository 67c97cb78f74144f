// codec_shape_dump.cpp — the launch rules of celestia-app_amd/csrc/codec_shape.h as a stand-alone host program, built
// and run under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_codec_shapes.py.  No device, no HIP.
//
// With no argument it answers the lines of its standard input, one line each:
//   dec k L ncw   ->  "dec k L ncw : PL m n log2n U slices lds_bytes"                 (launch_rs_decode)
//   enc8 k L ncw  ->  "enc8 k L ncw : lds log2m U slices lat lds_bytes"               (rs_encode8_kernel)
//                     "enc8 k L ncw : reg log2m slices lds_bytes"                     (rs_encode8_g2_kernel)
//   either        ->  "... : unsupported" where the launcher returns -2
// (enc8: ncw codewords of one block and the release value of lat_u, as cda_rs_encode_device launches them).
//
// With the argument "cells" it walks a domain and prints every distinct cell once, with the first input that reached
// it; a cell is what decides which code a kernel runs:
//   decoder      "D PL log2n U k<m : k L ncw"        k = 1..512, L = every multiple of 64 up to 2 KiB and of 1 KiB up
//                                                    to 512 KiB, ncw in {1, 2, 63, 64, 128, 256, 512, 1024}
//   LDS encoder  "E log2m U lat items>512 : k L ncw" k = 1..128, L = every multiple of 64 up to 4 KiB,
//                                                    ncw in {1, 2, 3, 64, 65, 66, 101}
// and over the whole domain checks what the kernels assume of a launch, a "V ..." line for each violation:
//   n * U <= 1024 (the decoder's four items per thread), U * slices * unit == L, lds_bytes within the cap set with
//   hipFuncSetAttribute, and no "unsupported" inside the domain.
// The last line is "checked <decoder shapes> <encoder shapes>".
#include <stdio.h>
#include <string.h>

#include <set>
#include <tuple>
#include <vector>

#include "../../celestia-app_amd/csrc/codec_shape.h"

using namespace cda;

static void answer_dec(int k, int L, int ncw) {
  const RsDecodeShape s = rs_decode_shape(k, L, ncw);
  if (!s.ok)
    printf("dec %d %d %d : unsupported\n", k, L, ncw);
  else
    printf("dec %d %d %d : %d %d %d %d %d %d %zu\n", k, L, ncw, s.PL, s.m, s.n, s.log2n, s.U, s.slices, s.lds_bytes);
}

static void answer_enc8(int k, int L, int ncw) {
  const RsEncode8Shape s = rs_encode8_shape(k, L, ncw, 1, kRs8LatU);
  if (!s.ok)
    printf("enc8 %d %d %d : unsupported\n", k, L, ncw);
  else if (s.reg)
    printf("enc8 %d %d %d : reg %d %d %zu\n", k, L, ncw, s.log2m, s.slices, s.lds_bytes);
  else
    printf("enc8 %d %d %d : lds %d %d %d %d %zu\n", k, L, ncw, s.log2m, s.U, s.slices, s.lat, s.lds_bytes);
}

static int answer_stdin() {
  char op[16];
  int k, L, ncw;
  for (;;) {
    const int got = scanf("%15s %d %d %d", op, &k, &L, &ncw);
    if (got == EOF) return 0;
    if (got != 4) return 2;
    if (!strcmp(op, "dec"))
      answer_dec(k, L, ncw);
    else if (!strcmp(op, "enc8"))
      answer_enc8(k, L, ncw);
    else
      return 2;
  }
}

static int walk_cells() {
  std::vector<int> dec_len, enc_len;
  for (int L = 64; L <= 2048; L += 64) dec_len.push_back(L);
  for (int L = 3072; L <= 512 * 1024; L += 1024) dec_len.push_back(L);
  for (int L = 64; L <= 4096; L += 64) enc_len.push_back(L);
  const int dec_ncw[] = {1, 2, 63, 64, 128, 256, 512, 1024};
  const int enc_ncw[] = {1, 2, 3, 64, 65, 66, 101};
  long long ndec = 0, nenc = 0;

  std::set<std::tuple<int, int, int, int>> seen;
  for (int k = 1; k <= 512; k++)
    for (int L : dec_len)
      for (int ncw : dec_ncw) {
        const RsDecodeShape s = rs_decode_shape(k, L, ncw);
        ndec++;
        if (!s.ok) {
          printf("V dec %d %d %d unsupported\n", k, L, ncw);
          continue;
        }
        const int unit = s.PL * 4;
        if (s.n * s.U > 1024) printf("V dec %d %d %d items %d\n", k, L, ncw, s.n * s.U);
        if ((long long)s.U * s.slices * unit != L) printf("V dec %d %d %d bytes %d %d\n", k, L, ncw, s.U, s.slices);
        if (s.lds_bytes > (size_t)kRsDecodeMaxLds) printf("V dec %d %d %d lds %zu\n", k, L, ncw, s.lds_bytes);
        if (s.m < k || s.m >= 2 * k || s.n != 2 * s.m || (1 << s.log2n) != s.n || (1 << s.log2U) != s.U)
          printf("V dec %d %d %d sizes %d %d %d %d\n", k, L, ncw, s.m, s.n, s.log2n, s.log2U);
        if (seen.insert({s.PL, s.log2n, s.U, k < s.m}).second)
          printf("D %d %d %d %d : %d %d %d\n", s.PL, s.log2n, s.U, (int)(k < s.m), k, L, ncw);
      }

  seen.clear();
  for (int k = 1; k <= 128; k++)
    for (int L : enc_len)
      for (int ncw : enc_ncw) {
        const RsEncode8Shape s = rs_encode8_shape(k, L, ncw, 1, kRs8LatU);
        nenc++;
        if (!s.ok) {
          printf("V enc8 %d %d %d unsupported\n", k, L, ncw);
          continue;
        }
        if (s.reg) {
          if (s.slices * 512 != L) printf("V enc8 %d %d %d reg bytes %d\n", k, L, ncw, s.slices);
          continue;
        }
        if ((long long)s.U * s.slices * 32 != L) printf("V enc8 %d %d %d bytes %d %d\n", k, L, ncw, s.U, s.slices);
        if (s.lds_bytes > (size_t)kRsEncode8MaxLds) printf("V enc8 %d %d %d lds %zu\n", k, L, ncw, s.lds_bytes);
        if (s.m < k || s.m >= 2 * k || (1 << s.log2m) != s.m || (1 << s.log2U) != s.U)
          printf("V enc8 %d %d %d sizes %d %d %d\n", k, L, ncw, s.m, s.log2m, s.log2U);
        const int second = s.m * s.U > 512;
        if (seen.insert({s.log2m, s.U, s.lat, second}).second)
          printf("E %d %d %d %d : %d %d %d\n", s.log2m, s.U, s.lat, second, k, L, ncw);
      }
  printf("checked %lld %lld\n", ndec, nenc);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 1) return answer_stdin();
  if (argc == 2 && !strcmp(argv[1], "cells")) return walk_cells();
  fprintf(stderr, "usage: codec_shape_dump [cells] (no argument: 'dec|enc8 k L ncw' lines on stdin)\n");
  return 2;
}
