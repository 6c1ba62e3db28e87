// Batched KZG evaluation audit (K13): verifySecret (DistSys/kyber.go:650-673) for every
// (chunk k, share point j) of a round's aggregate in ONE pairing-product check.
//
// The reference's check of one share is
//     e(C_k, g2_0) == e(W_kj, g2_1 - x_j G2) * e(B_k, g2_0)^y_kj
// (B_k = G1 in the reference's literal form, PK[poly*k] for a chunk-consistent check: quirk Q9).
// With independent random 64-bit weights r_kj all of them hold (up to a 2^-64 soundness error)
// iff
//     e(L1, g2_0) * e(-A, g2_1) * e(L2, G2) == 1,
//     L1 = sum_k (R_k C_k - Z_k B_k),  R_k = sum_j r_kj,  Z_k = sum_j r_kj y_kj  (exact, 192-bit),
//     A  = sum_kj r_kj W_kj,           L2 = sum_kj x_j r_kj W_kj.
// The G1 side -- nch*npts + 2*nch variable-base scalar multiplications and their sum -- is this
// file; the three-pairing product (fixed, prepared G2 points) is host work on a native thread
// (runtime/pairing.cpp), overlapped with the next round.
//
// MI355X mapping: one thread per scalar multiplication, 64-thread blocks (one wave, ~280 blocks
// for the MNIST aggregate so every CU gets work), binary double-and-add over the scalar's actual
// bit length (no table: the bases change every round), then a wave-level LDS tree of Jacobian
// additions per output and a one-block second pass over the block partials.  Scalars are
// shifted in registers (no dynamically indexed private arrays, so nothing spills to scratch).
#include <hip/hip_runtime.h>

#include "bn256_dev.h"

using namespace bn;

namespace {

constexpr int KZ_THREADS = 64;

// r = splitmix64(seed + (idx + 1) * golden) | 1 -- the host oracle (bindings.cpp kzg_r) matches
__device__ __forceinline__ unsigned long long kzg_r(unsigned long long seed, unsigned long long idx) {
  unsigned long long z = seed + (idx + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (z ^ (z >> 31)) | 1ull;
}

// 192-bit scalars: three named limbs, shifted in registers (an indexed limb array would be a run-time-indexed
// private array: scratch, see the header).  Two's complement where a sign is meant.
struct u192 {
  unsigned long long w0, w1, w2;
};

__device__ __forceinline__ void u192_neg(u192& z) {
  z.w0 = ~z.w0; z.w1 = ~z.w1; z.w2 = ~z.w2;
  z.w0 += 1;
  const unsigned long long c0 = z.w0 == 0;
  z.w1 += c0;
  z.w2 += (c0 && z.w1 == 0);
}

// z += r * y (signed y, every int64 included), modulo 2^192
__device__ __forceinline__ void u192_add_signed_product(u192& z, unsigned long long r, long long y) {
  const unsigned long long m = y < 0 ? 0ull - (unsigned long long)y : (unsigned long long)y;
  u192 p = {r * m, __umul64hi(r, m), 0};
  if (y < 0) u192_neg(p);
  z.w0 += p.w0;
  const unsigned long long c0 = z.w0 < p.w0;
  const unsigned long long t1 = z.w1 + p.w1;
  const unsigned long long c1 = t1 < z.w1;
  z.w1 = t1 + c0;
  const unsigned long long c1b = z.w1 < c0;
  z.w2 += p.w2 + c1 + c1b;
}

// z = |z|; returns whether z was negative
__device__ __forceinline__ bool u192_abs(u192& z) {
  const bool neg = z.w2 >> 63;
  if (neg) u192_neg(z);
  return neg;
}

__device__ __forceinline__ int u192_bits(const u192& k) {
  if (k.w2) return 192 - __clzll(k.w2);
  if (k.w1) return 128 - __clzll(k.w1);
  if (k.w0) return 64 - __clzll(k.w0);
  return 0;
}

__device__ __forceinline__ void u192_shl(u192& k, int sh) {
  while (sh >= 64) { k.w2 = k.w1; k.w1 = k.w0; k.w0 = 0; sh -= 64; }
  if (sh) {
    k.w2 = (k.w2 << sh) | (k.w1 >> (64 - sh));
    k.w1 = (k.w1 << sh) | (k.w0 >> (64 - sh));
    k.w0 <<= sh;
  }
}

// the step of a left-to-right chain: returns bit 191 and shifts left by one
__device__ __forceinline__ bool u192_shl1_top(u192& k) {
  const bool top = k.w2 >> 63;
  k.w2 = (k.w2 << 1) | (k.w1 >> 63); k.w1 = (k.w1 << 1) | (k.w0 >> 63); k.w0 <<= 1;
  return top;
}

// Left-aligns k (top bit at position 191) and takes that bit off; returns k's bit length, 0 for k = 0.
// A chain then starts from the base and runs bits - 1 steps.
__device__ __forceinline__ int u192_chain_start(u192& k) {
  const int nbits = u192_bits(k);
  if (nbits == 0) return 0;
  u192_shl(k, 192 - nbits);
  u192_shl1_top(k);
  return nbits;
}

// k * P for a 192-bit unsigned k, left to right over its bit length
__device__ __forceinline__ jac jac_mul_192(const jac& p, u192 k) {
  const int nbits = u192_chain_start(k);
  if (nbits == 0) return jac_inf();
  jac acc = p;   // the top bit
  for (int b = 1; b < nbits; ++b) {
    acc = jac_dbl_nocheck(acc);
    if (u192_shl1_top(k)) acc = jac_add(acc, p);
  }
  return acc;
}

// same with an affine base (mixed additions: 11 products instead of 16)
__device__ __forceinline__ jac aff_mul_192(const aff& q, u192 k) {
  if (aff_is_inf(q)) return jac_inf();
  const int nbits = u192_chain_start(k);
  if (nbits == 0) return jac_inf();
  jac acc;
  acc.x = q.x;
  acc.y = q.y;
  acc.z = fp_one();
  for (int b = 1; b < nbits; ++b) {
    acc = jac_dbl_nocheck(acc);
    if (u192_shl1_top(k)) acc = jac_add_aff(acc, q);
  }
  return acc;
}

// sum of one Jacobian point per lane of the block, result valid in lane 0
__device__ __forceinline__ jac block_sum(jac v, uint32_t* lds) {
  const int t = threadIdx.x;
  for (int s = KZ_THREADS / 2; s > 0; s >>= 1) {
    if (t >= s && t < 2 * s) st_jac(lds + (t - s) * 24, v);
    __syncthreads();
    if (t < s) v = jac_add(v, ld_jac(lds + t * 24));
    __syncthreads();
  }
  return v;
}

}  // namespace

// Threads [0, nch*npts): witness terms of (k, j) -> A += r W, L2 += x_j r W.
// Threads [nch*npts, +nch): R_k C_k -> L1.   Threads [nch*npts + nch, +nch): -Z_k B_k -> L1.
// wsum row of (k, j): (j / spm) * nch * spm + k * spm + j % spm (the miners' witness sums as the
// engine lays them out: contributing-miner-major, then chunk, then the miner's share slots).
// partial: [gridDim.x][3][24] Jacobian (L1, A, L2).
extern "C" __global__ void __launch_bounds__(KZ_THREADS) k_kzg_rlc(
    const uint32_t* __restrict__ csum, const uint32_t* __restrict__ wsum, const long long* __restrict__ ys,
    const int* __restrict__ xs, int nch, int npts, int spm, const uint32_t* __restrict__ bases, int base_stride,
    int nch_round, unsigned long long seed, uint32_t* __restrict__ partial) {
  __shared__ uint32_t lds[KZ_THREADS * 24];
  const long long g = (long long)blockIdx.x * KZ_THREADS + threadIdx.x;
  const long long nw = (long long)nch * npts;
  jac l1 = jac_inf(), a = jac_inf(), l2 = jac_inf();
  if (g < nw) {
    const int k = (int)(g / npts), j = (int)(g % npts);
    const unsigned long long r = kzg_r(seed, (unsigned long long)g);
    const long long row = (long long)(j / spm) * nch * spm + (long long)k * spm + j % spm;
    const jac w = ld_jac(wsum + row * 24);
    a = jac_mul_192(w, u192{r, 0, 0});
    const int x = xs[(long long)(k / nch_round) * npts + j];
    const unsigned ax = x < 0 ? unsigned(-x) : unsigned(x);
    l2 = jac_mul_192(a, u192{ax, 0, 0});
    if (x < 0) l2 = jac_neg(l2);
  } else if (g < nw + nch) {
    const int k = (int)(g - nw);
    u192 R = {0, 0, 0};   // R = sum_j r_kj: 128 bits
    for (int j = 0; j < npts; ++j) {
      const unsigned long long r = kzg_r(seed, (unsigned long long)k * npts + j);
      R.w0 += r;
      R.w1 += R.w0 < r;
    }
    l1 = jac_mul_192(ld_jac(csum + (long long)k * 24), R);
  } else if (g < nw + 2 * nch) {
    const int k = (int)(g - nw - nch);
    u192 Z = {0, 0, 0};   // Z = sum_j r_kj * y_kj
    for (int j = 0; j < npts; ++j)
      u192_add_signed_product(Z, kzg_r(seed, (unsigned long long)k * npts + j), ys[(long long)k * npts + j]);
    const bool neg = u192_abs(Z);
    const aff b = ld_aff(bases + (long long)(k % nch_round) * base_stride * 16);
    l1 = aff_mul_192(b, Z);
    if (!neg) l1 = jac_neg(l1);   // the term is -Z_k B_k
  }
  l1 = block_sum(l1, lds);
  a = block_sum(a, lds);
  l2 = block_sum(l2, lds);
  if (threadIdx.x == 0) {
    uint32_t* o = partial + (long long)blockIdx.x * 72;
    st_jac(o, l1);
    st_jac(o + 24, a);
    st_jac(o + 48, l2);
  }
}

// out[3][24] = sum over the nb block partials (one block)
extern "C" __global__ void __launch_bounds__(KZ_THREADS) k_kzg_reduce(const uint32_t* __restrict__ partial, int nb,
                                                                      uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[KZ_THREADS * 24];
  for (int s = 0; s < 3; ++s) {
    jac v = jac_inf();
    for (int i = threadIdx.x; i < nb; i += KZ_THREADS) v = jac_add(v, ld_jac(partial + (long long)i * 72 + s * 24));
    v = block_sum(v, lds);
    if (threadIdx.x == 0) st_jac(out + s * 24, v);
  }
}

// csum [nch][24], wsum [nch*npts][24] (layout above), ys int64 [nch][npts], xs int32 [nch/nch_round][npts],
// bases affine [*][16] read at (k % nch_round) * base_stride (0: one base for every chunk, the
// literal check).  Several rounds' aggregates stack as nch = rounds * nch_round chunks (witness
// sums pre-permuted to (chunk, point) order, spm = npts): the sums then cover all of them,
// one random weight per (round, chunk, point), and one launch serves the whole batch;
// partial scratch [blocks][72] (blocks = bsc_kzg_blocks), out [3][24] = (L1, A, L2).
extern "C" int bsc_kzg_blocks(int nch, int npts) {
  const long long n = (long long)nch * npts + 2LL * nch;
  return (int)((n + KZ_THREADS - 1) / KZ_THREADS);
}

extern "C" int bsc_kzg_rlc(const uint32_t* csum, const uint32_t* wsum, const long long* ys, const int* xs, int nch,
                           int npts, int spm, const uint32_t* bases, int base_stride, int nch_round,
                           unsigned long long seed, uint32_t* partial, uint32_t* out, void* stream) {
  if (nch <= 0 || npts <= 0) return 0;
  if (spm <= 0 || npts % spm != 0 || base_stride < 0 || npts > 4096 || nch_round <= 0 || nch % nch_round != 0)
    return -1;
  const int nb = bsc_kzg_blocks(nch, npts);
  hipLaunchKernelGGL(k_kzg_rlc, dim3(nb), dim3(KZ_THREADS), 0, (hipStream_t)stream, csum, wsum, ys, xs, nch, npts, spm,
                     bases, base_stride, nch_round, seed, partial);
  hipLaunchKernelGGL(k_kzg_reduce, dim3(1), dim3(KZ_THREADS), 0, (hipStream_t)stream, partial, nb, out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ per-row audit (--kzg-audit shares)
// The same triple for every row (worker update) of the share MSM's output on its own, read in place:
// pts [n][nch][T+1][24] (slots 0..T-1 the witnesses, slot T the chunk commitment), ys [n][nch][T].
// Row i draws its weights from its own seed s_i = kzg_r(seed, 2^40 + i), r_ikj = kzg_r(s_i, k*npts + j),
// so its triple is the aggregate audit's of (C_i, W_i, y_i) under s_i and the rows' sum is an RLC over all of them.
//
// MI355X mapping: n times the aggregate audit's chains, so the witness terms share their doublings.  A lane
// keeps one share point j and KR_M chunks; all its terms go through ONE accumulator, Straus fashion:
//     acc = 2 acc;  acc += W_k for every chunk k of the lane whose r_ikj has the bit set
// -- 64 doublings per lane instead of 64 per term, the weights recomputed from the seed (a few integer
// multiplications beside a 16-product addition) and the witnesses re-read from L1/L2 (24 KB per block), so the
// lane holds no table and indexes no private array.  x_j multiplies the lane's sum once at the end.  A wave
// holds 64 / npts groups of lanes over a slab of KR_M * groups chunks (a 64-thread block; (slab, row) grid:
// ~2300 witness blocks for MNIST's 35 rows x 785 chunks x 21 points).  R_ik C_ik - Z_ik B_k is one joint chain per
// chunk, 64 chunks per block, in blocks of their own behind the witness blocks.  One LDS tree per block
// output, then a block per row over the row's partials and k_kzg_reduce over the rows for the total.
namespace {

constexpr int KR_M = 4;   // chunks per lane: 8 + 16 KR_M products per bit instead of 24 KR_M

}  // namespace

// grid (nslab + nl1, n).  Blocks x < nslab: witness terms of chunks [x * slab, +slab) -> partial (A, L2);
// blocks x >= nslab: the commitment terms of chunks [(x - nslab) * 64, +64) -> partial (L1, -).
// partial [n][gridDim.x][2][24].  A row whose flag is 0 is not read (its blocks leave at once).
extern "C" __global__ void __launch_bounds__(KZ_THREADS) k_kzg_rows(
    const uint32_t* __restrict__ pts, const long long* __restrict__ ys, const int* __restrict__ alive,
    const int* __restrict__ cols, const int* __restrict__ xs, int nch, int T, int npts, int nslab,
    const uint32_t* __restrict__ bases, int base_stride, unsigned long long seed, uint32_t* __restrict__ partial) {
  __shared__ uint32_t lds[KZ_THREADS * 24];
  const int i = blockIdx.y, bx = blockIdx.x, t = threadIdx.x;
  if (alive != nullptr && alive[i] == 0) return;   // block-uniform
  const unsigned long long s = kzg_r(seed, (1ull << 40) + (unsigned long long)i);
  const long long cstride = (long long)(T + 1) * 24;
  const uint32_t* prow = pts + (long long)i * nch * cstride;
  const long long* yrow = ys + (long long)i * nch * T;
  jac u = jac_inf(), v = jac_inf();
  if (bx < nslab) {
    const int G = KZ_THREADS / npts;
    const int g = t / npts, j = t % npts;
    const int c = t < G * npts ? cols[j] : -1;
    if ((unsigned)c < (unsigned)T) {   // (a column outside the row's slots contributes nothing: the check then fails)
      const int k0 = bx * G * KR_M + g;
      const uint32_t* w0 = prow + (long long)c * 24;
      for (int b = 63; b >= 0; --b) {
        u = jac_dbl_nocheck(u);
#pragma unroll 1
        for (int m = 0; m < KR_M; ++m) {
          const int k = k0 + m * G;
          if (k < nch) {
            const unsigned long long r = kzg_r(s, (unsigned long long)k * npts + j);
            if ((r >> b) & 1ull) u = jac_add(u, ld_jac(w0 + (long long)k * cstride));
          }
        }
      }
      const int x = xs[j];
      const unsigned ax = x < 0 ? unsigned(-x) : unsigned(x);
      v = jac_mul_192(u, u192{ax, 0, 0});
      if (x < 0) v = jac_neg(v);
    }
  } else {
    const int k = (bx - nslab) * KZ_THREADS + t;
    if (k < nch) {
      // R = sum_j r (128-bit), Z = sum_j r * y (two's complement over 192 bits)
      u192 R = {0, 0, 0}, Z = {0, 0, 0};
      for (int j = 0; j < npts; ++j) {
        const int c = cols[j];
        if ((unsigned)c >= (unsigned)T) continue;
        const unsigned long long r = kzg_r(s, (unsigned long long)k * npts + j);
        R.w0 += r;
        R.w1 += R.w0 < r;
        u192_add_signed_product(Z, r, yrow[(long long)k * T + c]);
      }
      const bool neg = u192_abs(Z);
      const jac C = ld_jac(prow + (long long)k * cstride + (long long)T * 24);
      aff B = ld_aff(bases + (long long)k * base_stride * 16);
      if (!neg) B = aff_neg(B);   // the term is -Z B
      // R C + |Z| (+-B): one chain over the longer scalar, both left-aligned at bit 191
      const int nr = u192_bits(R), nz = u192_bits(Z);
      const int nbits = nr > nz ? nr : nz;
      u192_shl(R, 192 - nbits);
      u192_shl(Z, 192 - nbits);
      for (int b = 0; b < nbits; ++b) {
        u = jac_dbl_nocheck(u);
        if (u192_shl1_top(R)) u = jac_add(u, C);
        if (u192_shl1_top(Z)) u = jac_add_aff(u, B);
      }
    }
  }
  u = block_sum(u, lds);
  if (bx < nslab) v = block_sum(v, lds);
  if (t == 0) {
    uint32_t* o = partial + ((long long)i * gridDim.x + bx) * 48;
    st_jac(o, u);
    st_jac(o + 24, v);
  }
}

// out[i] = (L1, A, L2) of row i from its block partials, one block per row; three infinities for a skipped row
extern "C" __global__ void __launch_bounds__(KZ_THREADS) k_kzg_rows_reduce(const uint32_t* __restrict__ partial,
                                                                           const int* __restrict__ alive, int nslab,
                                                                           int nb, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[KZ_THREADS * 24];
  const int i = blockIdx.x, t = threadIdx.x;
  const bool on = alive == nullptr || alive[i] != 0;   // block-uniform
  const uint32_t* p = partial + (long long)i * nb * 48;
  for (int s = 0; s < 3; ++s) {
    jac v = jac_inf();
    if (on) {
      // L1: the first point of the commitment blocks; A, L2: the two points of the witness blocks
      const int lo = s == 0 ? nslab : 0, hi = s == 0 ? nb : nslab;
      for (int b = lo + t; b < hi; b += KZ_THREADS) v = jac_add(v, ld_jac(p + (long long)b * 48 + (s == 2 ? 24 : 0)));
      v = block_sum(v, lds);
    }
    if (t == 0) st_jac(out + (long long)i * 72 + s * 24, v);
  }
}

// Blocks of one row (witness slabs, commitment blocks) for bsc_kzg_rlc_rows' partial scratch [n][blocks][48].
extern "C" int bsc_kzg_rows_blocks(int nch, int npts) {
  if (nch <= 0 || npts <= 0 || npts > 32) return 0;
  const int slab = (KZ_THREADS / npts) * KR_M;
  return (nch + slab - 1) / slab + (nch + KZ_THREADS - 1) / KZ_THREADS;
}

// pts int32 [n][nch][T+1][24], ys int64 [n][nch][T] (a view of the share MSM's ring: native strides), alive int32 [n]
// or null, cols / xs int32 [npts] (share slots and their x, npts <= 32), bases affine as in bsc_kzg_rlc (nch_round =
// nch), partial [n * bsc_kzg_rows_blocks][48], out [n + 1][3][24]: row i's (L1, A, L2), row n their sums.
extern "C" int bsc_kzg_rlc_rows(const uint32_t* pts, const long long* ys, const int* alive, const int* cols,
                                const int* xs, int n, int nch, int T, int npts, const uint32_t* bases, int base_stride,
                                unsigned long long seed, uint32_t* partial, uint32_t* out, void* stream) {
  if (n < 0 || nch < 0 || npts < 0) return -1;
  if (n == 0 || npts == 0 || nch == 0) return 0;
  if (npts > 32 || T <= 0 || npts > T || base_stride < 0 || n > 65535) return -1;
  if (!pts || !ys || !cols || !xs || !bases || !partial || !out) return -1;
  const int slab = (KZ_THREADS / npts) * KR_M;
  const int nslab = (nch + slab - 1) / slab;
  const int nb = bsc_kzg_rows_blocks(nch, npts);
  hipLaunchKernelGGL(k_kzg_rows, dim3(nb, n), dim3(KZ_THREADS), 0, (hipStream_t)stream, pts, ys, alive, cols, xs, nch, T,
                     npts, nslab, bases, base_stride, seed, partial);
  hipLaunchKernelGGL(k_kzg_rows_reduce, dim3(n), dim3(KZ_THREADS), 0, (hipStream_t)stream, partial, alive, nslab, nb,
                     out);
  hipLaunchKernelGGL(k_kzg_reduce, dim3(1), dim3(KZ_THREADS), 0, (hipStream_t)stream, out, n, out + (long long)n * 72);
  return (int)hipGetLastError();
}
