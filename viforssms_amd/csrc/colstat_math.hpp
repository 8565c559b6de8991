// Shared math of the column statistics (colstat.hip; include/vissm.h vissm_col_*): the order-preserving key of an
// fp32 value, its inverse, and one narrowing step of the byte-wise radix select.  __host__ __device__, so the CPU
// test-suite checks the very code the kernels run (hostcheck.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VISSM_HD __host__ __device__
#else
#define VISSM_HD
#endif

namespace vissm {
namespace cs {

constexpr uint32_t kNanKey = 0xFFFFFFFFu;

// Unsigned order of the keys = numpy's sort order of the floats: -inf .. -0 = +0 .. +inf, every NaN last.
VISSM_HD inline uint32_t key_of_bits(uint32_t b) {
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return kNanKey;  // NaN of either sign
  if (b == 0x80000000u) b = 0u;                         // -0 -> +0
  return (b >> 31) ? ~b : (b | 0x80000000u);
}

VISSM_HD inline uint32_t bits_of_key(uint32_t k) {
  if (k == kNanKey) return 0x7FC00000u;  // quiet NaN
  return (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
}

VISSM_HD inline uint32_t float_bits(float x) {
  uint32_t b;
  memcpy(&b, &x, sizeof b);
  return b;
}

VISSM_HD inline float bits_float(uint32_t b) {
  float x;
  memcpy(&x, &b, sizeof x);
  return x;
}

VISSM_HD inline uint32_t colkey(float x) { return key_of_bits(float_bits(x)); }
VISSM_HD inline float colkey_inv(uint32_t k) { return bits_float(bits_of_key(k)); }

// key byte examined by pass 0..3 (most significant first)
VISSM_HD inline int pass_shift(int pass) { return 8 * (3 - pass); }

// the part of a key above the byte of `pass` (0 in pass 0: every element matches)
VISSM_HD inline uint32_t key_above(uint32_t key, int pass) { return pass == 0 ? 0u : key >> (pass_shift(pass) + 8); }

// One narrowing step on the 256-bin histogram of one (column, target): the digit d with
// cum[d-1] <= rank_left < cum[d]; rank_left -= cum[d-1]; prefix |= d << shift.  A rank outside [0, total) is
// clamped to the nearest valid one (the host entry points refuse such ranks where they can see them), so the step
// ends on an occupied bin whatever it is given; an empty histogram leaves digit 0.
VISSM_HD inline void col_narrow(const int32_t* hist, int32_t* rank_left, uint32_t* prefix, int pass) {
  int32_t total = 0;
  for (int d = 0; d < 256; ++d) total += hist[d];
  int32_t r = *rank_left;
  if (r > total - 1) r = total - 1;
  if (r < 0) r = 0;
  int32_t below = 0;
  int digit = 0;
  for (int d = 0; d < 256; ++d) {
    const int32_t h = hist[d];
    if (h > 0 && r < below + h) {
      digit = d;
      break;
    }
    below += h;
  }
  *rank_left = r - below;
  *prefix |= static_cast<uint32_t>(digit) << pass_shift(pass);
}

}  // namespace cs
}  // namespace vissm
