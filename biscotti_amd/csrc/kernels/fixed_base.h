// Window plan of every fixed-base table (msm.hip, schnorr.hip; ops/bn256.py fb_entries is the one Python copy).
//
// A base's table holds the multiples a signed-digit scalar multiplication needs: window 0 is B0 bits wide
// (E0 = 2^(B0-1) entries: signed digits |d| <= 2^(B0-1)), windows 1..NW-1 are 8 bits (FB_ENTRIES = 128 each).
// Per base the entries are laid out window 0 first, then 128 per further window, PB = E0 + 128 (NW - 1) in
// all; entry (w, |d|) holds |d| * 2^shift_w * base with shift_0 = 0, shift_w = B0 + 8 (w - 1).
// A wide first window turns the typical quantised update coefficient (|q| < 2^13) into ONE mixed addition
// instead of two: HBM is spent (tens of GB of tables) to halve the MSM arithmetic.
//
// Every lane of an MSM indexes those tables with the numbers below, so they are written once: plain C++ for
// host and device (the launchers' argument checks, the kernels' indexing, and csrc/selftest under g++).
#pragma once

#if defined(__HIPCC__)
#define BSC_HD __host__ __device__
#else
#define BSC_HD
#endif

constexpr int FB_ENTRIES = 128;   // entries of an 8-bit signed window

struct FbPlan {
  int B0, NW;     // bits of window 0, number of windows
  int E0;         // entries of window 0
  long long PB;   // entries per base
};

// B0 in [8, 20] (window 0 is a whole number of 128-entry runs, E0 fits an int) and at least one window
BSC_HD constexpr bool fb_plan_ok(int B0, int NW) { return B0 >= 8 && B0 <= 20 && NW >= 1; }
// ... and the windows cover every int64 scalar with its recoding carry: what an MSM over coefficients needs
BSC_HD constexpr bool fb_covers_i64(int B0, int NW) { return fb_plan_ok(B0, NW) && B0 + 8 * (NW - 1) >= 65; }

// (B0, NW) must be fb_plan_ok
BSC_HD constexpr FbPlan fb_plan(int B0, int NW) {
  return FbPlan{B0, NW, 1 << (B0 - 1), (long long)(1 << (B0 - 1)) + (long long)(NW - 1) * FB_ENTRIES};
}

// 128-entry runs per base (k_fb_table builds one run per thread): E0 / 128 of window 0, one per further window
BSC_HD constexpr int fb_runs(const FbPlan& p) { return p.E0 / FB_ENTRIES + p.NW - 1; }
BSC_HD constexpr int fb_window_bits(const FbPlan& p, int w) { return w ? 8 : p.B0; }
BSC_HD constexpr int fb_window_shift(const FbPlan& p, int w) { return w ? p.B0 + 8 * (w - 1) : 0; }
// entry index of (window w, |digit| ad >= 1) inside a base, in [0, PB)
BSC_HD constexpr int fb_entry(const FbPlan& p, int w, int ad) {
  return (w ? p.E0 + (w - 1) * FB_ENTRIES : 0) + ad - 1;
}

// next signed digit of width `bits` from (m, carry); digits lie in (-2^(bits-1), 2^(bits-1)]
BSC_HD __attribute__((always_inline)) inline int fb_next_digit(unsigned long long& m, int& carry, int bits) {
  int dg = (int)(m & ((1ull << bits) - 1)) + carry;
  m >>= bits;
  if (dg > (1 << (bits - 1))) {
    dg -= 1 << bits;
    carry = 1;
  } else {
    carry = 0;
  }
  return dg;
}

// The signed-digit walk of c * base: f(w, ad, negate) once per nonzero digit, lowest window first; the term
// is entry (w, ad) of the base, negated when the digit's sign and c's differ.
template <class F>
BSC_HD __attribute__((always_inline)) inline void fb_walk(long long c, const FbPlan& p, F&& f) {
  const bool neg = c < 0;
  unsigned long long m = neg ? 0ull - (unsigned long long)c : (unsigned long long)c;
  int carry = 0;
  for (int w = 0; w < p.NW && (m != 0 || carry != 0); ++w) {
    const int dg = fb_next_digit(m, carry, fb_window_bits(p, w));
    if (dg == 0) continue;
    f(w, dg < 0 ? -dg : dg, (dg < 0) != neg);
  }
}
