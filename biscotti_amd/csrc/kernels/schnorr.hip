// Batched Schnorr verification over BN256 G1 on gfx950: the verifier signatures of a round (--verify-signatures,
// main.go:269-277, Q5) and their opt-in audit (--sig-audit).  The host verifier is the specification
// (runtime/bn256.cpp schnorr_verify, hash_schnorr, pick_scalar_from_xof; runtime/hash.cpp Blake2Xb;
// the reference: DistSys/kyber.go:873-933).
//
// A signature is c || r (two 32-byte big-endian scalars) over a 64-byte message.  It is valid iff c < n, r < n
// and c == H(marshal(r G + c PK) || message), H = the first BLAKE2Xb candidate v with 0 < v < n, the XOF keyed
// with the 64-byte marshal of T = r G + c PK.
//
// Signing (k_schnorr_sign; the host signer schnorr_sign / run_sign_job is the specification): the nonce v is the
// first candidate of the same XOF keyed with 36 bytes of entropy (the signer's nonce base || le32(nonce id)) and
// given no message; T = v G, c = H(marshal(T) || message), r = v - sk c mod n.  One fixed-base product where the
// verifier has two; the same 64 bytes as the host.  Its statuses: 0 signed | 3 | 4, as below.
//
// Status of an item (msg_idx, key_idx, signature), the first failing check decides:
//   0 valid | 1 c >= n or r >= n | 2 the recomputed challenge differs | 3 undecided after DRAWS candidates (the
//   host decides) | 4 msg_idx or key_idx out of range
//
// Shape: the work of one item is latency -- 66 dependent mixed additions, one Fermat inversion, ~4 BLAKE2b
// compressions.  One workgroup is one wave of 16 items x 4 lanes; lane (p, q) of item p sums
//   q = 0: r G windows 0..16 | q = 1: r G windows 17..32 | q = 2: c PK windows 0..16 | q = 3: c PK windows 17..32
// over the fixed-base tables (the four lanes run the same code on different table rows: no divergence but the
// digits' own).  The four partial Jacobian sums are handed over in LDS; lane q = 0 then adds them (3 additions),
// inverts once, marshals, hashes and writes the status.  Lanes of a failed or out-of-range item walk every barrier;
// no thread returns before the last one.
//
// Tables (built by k_fb_table, msm.hip): B0 = 8, NW = 33, layout [base][entry][16], entry (w, |d|) of a base at
// w * 128 + |d| - 1 holding |d| * 2^(8 w) * base (affine, Montgomery; (0, 0) = infinity).  Base 0 is G, base
// 1 + k is peer key k.  33 windows: a scalar below n still has a top byte up to 0x8F, so its signed 8-bit
// recoding can carry out of window 31.
//
// Memory safety -- keep these true:
//  * Table reads: window w in [0, 32] (the loop's guard); digit d in [-127, 128] from recode8, the one recoding
//    routine, which cannot give another value for a byte in [0, 255] and a carry in {0, 1}; window 32 has no byte
//    of its own, its digit is the last carry, 0 or 1.  Entry index w * 128 + |d| - 1 in [0, 4223] = [0, PB).
//    Base = 0 or key_idx + 1 in [1, nkeys].  In the verifier a scalar is recoded only after it passed < n.
//  * msg_idx and key_idx are compared against nmsg / nkeys before any address is formed from them; an
//    out-of-range item reads only its own 64 signature bytes.
//  * There are no per-thread arrays with a run-time bound or a run-time index: the scalars' bytes are read from
//    LDS, the BLAKE2b state and message words are named by literals.  The draw loop is bounded by DRAWS.
//  * A wrong answer comes out as a status, never as an access outside a buffer.
//  * The signer (k_schnorr_sign): msg_idx and key_idx are compared against nmsg / nkeys before a message, a key
//    row or a nonce base is addressed; an out-of-range item reads only its own three index words.  The nonce is a
//    XOF candidate, so it lies in (0, n) and recodes inside the table like a checked scalar; it reads base 0 only,
//    windows 0..8 | 9..16 | 17..24 | 25..32 per lane (window_sum's guard w < SNW holds for any split).  The nonce's
//    bytes come from LDS, the CIOS limbs and the BLAKE2b words are named by literals; both draw loops are the one
//    loop bounded by DRAWS.  Every thread walks both barriers: an item that is out of range or found no nonce
//    stores the point at infinity and its lane 0 writes a status (4 or 3) and 64 zero bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bn256_dev.h"
#include "fixed_base.h"

using namespace bn;

namespace {

constexpr int SP = 16;                // items per workgroup (one wave: 16 items x 4 lanes)
constexpr int DRAWS = 32;             // candidate draws at most (16 output nodes): missed with 0.439^32 ~ 3.5e-12
constexpr int SNW = 33;               // windows per base
constexpr int SPB = SNW * 128;        // entries per base
static_assert(SPB == fb_plan(8, SNW).PB, "the verifier's table is the (B0 = 8, NW = 33) plan of fixed_base.h");
constexpr int HALF = 17;              // windows of a lane: 0..16, 17..32 (the second half has 16)

typedef unsigned long long u64;

// the group order n, little-endian 64-bit limbs
__constant__ static const u64 ORD[4] = {0x1a2ef45b57ac7261ull, 0x2e8d8e12f82b3924ull, 0xaa6fecb86184dc21ull,
                                        0x8fb501e34aa387f9ull};
__constant__ static const u64 B2IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                                         0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                                         0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};

__device__ __forceinline__ u64 rotr64(u64 x, int n) { return (x >> n) | (x << (64 - n)); }

// ---------------------------------------------------------------- BLAKE2b
// One compression of a block whose words 8..15 are zero (every block hashed here is 64 bytes of data in a
// 128-byte block): h the chained state, m the eight message words, t the byte counter (< 2^64), last the
// finalisation flag.  State and message words are named by literals only, so they stay in registers.
#define B2M(i) ((i) < 8 ? m[(i) & 7] : 0ull)
#define B2G(a, b, c, d, x, y)                                   \
  v[a] = v[a] + v[b] + (x); v[d] = rotr64(v[d] ^ v[a], 32);     \
  v[c] = v[c] + v[d];       v[b] = rotr64(v[b] ^ v[c], 24);     \
  v[a] = v[a] + v[b] + (y); v[d] = rotr64(v[d] ^ v[a], 16);     \
  v[c] = v[c] + v[d];       v[b] = rotr64(v[b] ^ v[c], 63);
#define B2ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
  B2G(0, 4, 8, 12, B2M(s0), B2M(s1))                                                   \
  B2G(1, 5, 9, 13, B2M(s2), B2M(s3))                                                   \
  B2G(2, 6, 10, 14, B2M(s4), B2M(s5))                                                  \
  B2G(3, 7, 11, 15, B2M(s6), B2M(s7))                                                  \
  B2G(0, 5, 10, 15, B2M(s8), B2M(s9))                                                  \
  B2G(1, 6, 11, 12, B2M(s10), B2M(s11))                                                \
  B2G(2, 7, 8, 13, B2M(s12), B2M(s13))                                                 \
  B2G(3, 4, 9, 14, B2M(s14), B2M(s15))
__device__ __forceinline__ void b2_compress(u64 (&h)[8], const u64 (&m)[8], u64 t, bool last) {
  u64 v[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    v[i] = h[i];
    v[i + 8] = B2IV[i];
  }
  v[12] ^= t;
  if (last) v[14] = ~v[14];
  B2ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  B2ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
  B2ROUND(11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4)
  B2ROUND(7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8)
  B2ROUND(9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13)
  B2ROUND(2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9)
  B2ROUND(12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11)
  B2ROUND(13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10)
  B2ROUND(6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5)
  B2ROUND(10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0)
  B2ROUND(0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
  B2ROUND(14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3)
#pragma unroll
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
}
#undef B2ROUND
#undef B2G
#undef B2M

// The challenge of hash_schnorr: BLAKE2Xb keyed with `key` (T's marshal, 64 bytes as eight little-endian words)
// over `msg` (64 bytes, likewise), read 32 bytes at a time; the first candidate v with 0 < v < n, as four
// little-endian 64-bit limbs in out.  Returns the candidates drawn (1..DRAWS), or 0 when none of DRAWS fits.
//   root node  : parameter block digest 64, key 64, fanout 1, depth 1, bytes 12..15 = 0xFF; input the key block
//                (t = 128) and the message as the final block (t = 192)
//   output node i: digest 64, key 0, fanout 0, depth 0, leaf length 64, node offset i, bytes 12..15 = 0xFF, inner
//                length 64; input the root digest, final (t = 64)
//   candidate j: bytes 32 (j mod 2) .. +31 of node j div 2, big-endian
// The signer's nonce (schnorr_nonce) is the same XOF keyed with 36 bytes of entropy and given no message: its root
// node is the key block alone, final (t = 128), under a parameter block whose key length is 36.
// One rolled loop holds the single inlined copy of the compression: steps 0 and 1 are the root node's two
// blocks (step 1 is skipped when there is no message), step 2 + i is output node i.  p0: the first word of the
// root's parameter block; key: the key block's first 64 bytes (the rest is zero).
constexpr u64 XOF_KEY64 = 0x0000000001014040ull;   // digest 64, key 64, fanout 1, depth 1
constexpr u64 XOF_KEY36 = 0x0000000001012440ull;   // digest 64, key 36, fanout 1, depth 1
__device__ __forceinline__ int schnorr_xof(u64 p0, const u64 (&key)[8], bool has_msg, const u64 (&msg)[8],
                                           u64 (&out)[4]) {
  u64 st[8], root[8], m[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) root[i] = 0;
  int used = 0;
#pragma unroll 1
  for (int step = 0; step < 2 + DRAWS / 2; ++step) {
    u64 t;
    bool last;
    if (step == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        st[i] = B2IV[i];
        m[i] = key[i];
      }
      st[0] ^= p0;
      st[1] ^= 0xFFFFFFFF00000000ull;
      t = 128;
      last = !has_msg;
    } else if (step == 1) {
#pragma unroll
      for (int i = 0; i < 8; ++i) m[i] = msg[i];
      t = 192;
      last = true;
    } else {
      if (step == 2) {
#pragma unroll
        for (int i = 0; i < 8; ++i) root[i] = st[i];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        st[i] = B2IV[i];
        m[i] = root[i];
      }
      st[0] ^= 0x0000004000000040ull;
      st[1] ^= 0xFFFFFFFF00000000ull | (u64)(uint32_t)(step - 2);
      st[2] ^= 0x0000000000004000ull;
      t = 64;
      last = true;
    }
    b2_compress(st, m, t, last);
    if (step == 0 && !has_msg) step = 1;   // the root node was that one block
    if (step >= 2) {
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        if (used == 0) {
          u64 v[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = __builtin_bswap64(st[4 * half + 3 - j]);
          const bool nz = (v[0] | v[1] | v[2] | v[3]) != 0;
          bool lt = false;   // v < n
#pragma unroll
          for (int j = 0; j < 4; ++j) {   // from the least significant limb up: the highest differing limb decides
            if (v[j] != ORD[j]) lt = v[j] < ORD[j];
          }
          if (nz && lt) {
            used = 2 * (step - 2) + half + 1;
#pragma unroll
            for (int j = 0; j < 4; ++j) out[j] = v[j];
          }
        }
      }
      if (used) break;
    }
  }
  return used;
}
__device__ __forceinline__ int schnorr_challenge(const u64 (&key)[8], const u64 (&msg)[8], u64 (&out)[4]) {
  return schnorr_xof(XOF_KEY64, key, true, msg, out);
}

// ---------------------------------------------------------------- scalars and points
__device__ __forceinline__ uint32_t ld_be32(const uint32_t* p) { return __builtin_bswap32(*p); }

// 32 big-endian bytes (4-byte aligned) -> eight little-endian 32-bit limbs
__device__ __forceinline__ void ld_scalar_be(uint32_t (&k)[8], const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = ld_be32(p + 7 - i);
}
__device__ __forceinline__ bool scalar_lt_n(const uint32_t (&k)[8]) {
  bool lt = false;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u64 v = ((u64)k[2 * j + 1] << 32) | k[2 * j];
    if (v != ORD[j]) lt = v < ORD[j];
  }
  return lt;
}

// The one recoding routine: the next signed 8-bit digit of a scalar from its byte (0..255) and the carry (0 or 1)
// of the windows below; the result lies in [-127, 128] and the new carry in {0, 1}.  For byte = 0 (window 32, which
// has no byte) the digit is the carry itself and the carry out is 0.
__device__ __forceinline__ int recode8(int byte, int& carry) {
  int d = (byte & 0xff) + (carry & 1);   // 0..256
  if (d > 128) {
    d -= 256;                            // -127..0
    carry = 1;
  } else {
    carry = 0;
  }
  return d;
}

// One lane's share of a fixed-base product: the sum over windows w0 .. min(w0 + cnt, SNW) - 1 of digit(w) * 2^(8 w)
// * base.  sc: the scalar's eight little-endian limbs in LDS (a run-time index is a plain address there); tb: the
// base's SPB entries of 16 words.  The carry into w0 comes from recoding the windows below it.
__device__ __forceinline__ jac window_sum(const uint32_t* sc, const uint32_t* __restrict__ tb, int w0, int cnt) {
  jac acc = jac_inf();
  int carry = 0;
  for (int w = 0; w < w0; ++w) (void)recode8((int)(sc[w >> 2] >> (8 * (w & 3))), carry);   // the carry into w0
#pragma unroll 1
  for (int j = 0; j < cnt; ++j) {
    const int w = w0 + j;
    if (w < SNW) {                                 // w in [0, 32]
      const int byte = w < 32 ? (int)((sc[w >> 2] >> (8 * (w & 3))) & 0xffu) : 0;
      const int d = recode8(byte, carry);          // [-127, 128]; window 32: 0 or 1
      if (d != 0) {
        const int ad = d < 0 ? -d : d;             // [1, 128]
        aff e = ld_aff(tb + 16 * (w * 128 + ad - 1));   // entry in [0, SPB)
        if (d < 0) e = aff_neg(e);
        acc = jac_add_aff(acc, e);
      }
    }
  }
  return acc;
}

// Phases 0 and 1 of the verifier and of bsc_schnorr_point, called by every thread of the workgroup (two barriers).
// act: this lane's item takes part (the four lanes of an item agree); r / c: its scalars (little-endian limbs);
// key: its peer key index, already checked to lie in [0, nkeys) when act.  On return s_part[q][p] holds lane
// (p, q)'s partial sum (infinity for an item that takes no part).
__device__ __forceinline__ void partial_sums(bool act, const uint32_t (&r)[8], const uint32_t (&c)[8], int key,
                                             const uint32_t* __restrict__ table, int p, int q,
                                             uint32_t (*s_sc)[2][8], uint32_t (*s_part)[SP][24]) {
  if (q == 0 || q == 2) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s_sc[p][q >> 1][i] = q == 0 ? r[i] : c[i];
  }
  __syncthreads();
  jac acc = jac_inf();
  if (act) {
    const int which = q >> 1;                        // 0: r G, 1: c PK
    const long long base = which ? (long long)key + 1 : 0;
    acc = window_sum(&s_sc[p][which][0], table + 16 * base * SPB, (q & 1) ? HALF : 0, HALF);
  }
  st_jac(&s_part[q][p][0], acc);
  __syncthreads();
}

// T = the four partial sums of item p; its marshal (x || y big-endian, out of Montgomery form; infinity: zeros)
// as the eight little-endian 64-bit words of the 64 bytes
__device__ __forceinline__ void marshal_sum(int p, uint32_t (*s_part)[SP][24], u64 (&out)[8]) {
  const jac a = jac_add(ld_jac(&s_part[0][p][0]), ld_jac(&s_part[1][p][0]));
  const jac b = jac_add(ld_jac(&s_part[2][p][0]), ld_jac(&s_part[3][p][0]));
  const aff t = jac_to_aff(jac_add(a, b));           // infinity -> (0, 0)
  const fp x = fp_from_mont(t.x), y = fp_from_mont(t.y);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    out[k] = (u64)__builtin_bswap32(x.v[7 - 2 * k]) | ((u64)__builtin_bswap32(x.v[6 - 2 * k]) << 32);
    out[4 + k] = (u64)__builtin_bswap32(y.v[7 - 2 * k]) | ((u64)__builtin_bswap32(y.v[6 - 2 * k]) << 32);
  }
}

// 64 bytes at p (4-byte aligned) as eight little-endian 64-bit words
__device__ __forceinline__ void ld_words64(u64 (&m)[8], const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < 8; ++i) m[i] = (u64)p[2 * i] | ((u64)p[2 * i + 1] << 32);
}
__device__ __forceinline__ void st_words64(uint32_t* p, const u64 (&m)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    p[2 * i] = (uint32_t)m[i];
    p[2 * i + 1] = (uint32_t)(m[i] >> 32);
  }
}

// ---------------------------------------------------------------- the signer's scalars (mod n)
constexpr uint32_t ORD_N0INV = 0x2d284e5fu;   // -n^-1 mod 2^32
__device__ __forceinline__ uint32_t ord32(int i) { return (uint32_t)(ORD[i >> 1] >> (32 * (i & 1))); }

// The response r = v - sk c mod n.  v, c: scalars below n; skr = sk 2^256 mod n, so that one Montgomery
// multiplication (8 x 32-bit CIOS, modulus n) by c gives sk c mod n; then a subtraction with conditional add-back.
// All limbs little-endian; every array index is a literal after unrolling.
__device__ __forceinline__ void schnorr_response(const uint32_t (&v)[8], const uint32_t (&skr)[8],
                                                 const uint32_t (&c)[8], uint32_t (&r)[8]) {
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    u64 cur, carry = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      cur = (u64)skr[j] * c[i] + t[j] + carry;
      t[j] = (uint32_t)cur;
      carry = cur >> 32;
    }
    cur = (u64)t[8] + carry;
    t[8] = (uint32_t)cur;
    t[9] = (uint32_t)(cur >> 32);
    const uint32_t m = t[0] * ORD_N0INV;
    cur = (u64)m * ord32(0) + t[0];
    carry = cur >> 32;
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      cur = (u64)m * ord32(j) + t[j] + carry;
      t[j - 1] = (uint32_t)cur;
      carry = cur >> 32;
    }
    cur = (u64)t[8] + carry;
    t[7] = (uint32_t)cur;
    t[8] = t[9] + (uint32_t)(cur >> 32);
  }
  // t < 2 n: x = t - n when t >= n
  uint32_t x[8];
  u64 borrow = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u64 d = (u64)t[j] - ord32(j) - borrow;
    x[j] = (uint32_t)d;
    borrow = (d >> 32) & 1;
  }
  const bool keep = t[8] == 0 && borrow != 0;   // t < n
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = keep ? t[j] : x[j];
  // r = v - x, + n when it borrows
  borrow = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u64 d = (u64)v[j] - x[j] - borrow;
    r[j] = (uint32_t)d;
    borrow = (d >> 32) & 1;
  }
  const uint32_t back = borrow ? 0xffffffffu : 0u;
  u64 carry = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u64 s = (u64)r[j] + (ord32(j) & back) + carry;
    r[j] = (uint32_t)s;
    carry = s >> 32;
  }
}

// four little-endian 64-bit limbs <-> eight 32-bit ones
__device__ __forceinline__ void limbs32(uint32_t (&k)[8], const u64 (&v)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    k[2 * j] = (uint32_t)v[j];
    k[2 * j + 1] = (uint32_t)(v[j] >> 32);
  }
}
// a scalar's 32 big-endian bytes as four little-endian 64-bit words of the byte string
__device__ __forceinline__ void scalar_be_words(u64 (&w)[4], const uint32_t (&k)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = __builtin_bswap64(((u64)k[7 - 2 * j] << 32) | k[6 - 2 * j]);
}

// 36 bytes of nonce entropy = the signer's 32-byte base (4-byte aligned) and the little-endian nonce id, as the
// key block's words
__device__ __forceinline__ void ld_entropy(u64 (&m)[8], const uint32_t* base, uint32_t id) {
#pragma unroll
  for (int i = 0; i < 4; ++i) m[i] = (u64)base[2 * i] | ((u64)base[2 * i + 1] << 32);
  m[4] = id;
  m[5] = m[6] = m[7] = 0;
}

}  // namespace

// messages: uint8 [nmsg][64]; msg_idx, key_idx: int [n]; sigs: uint8 [n][64] (c || r); table: [1 + nkeys][SPB][16]
// words; status: int [n]; counter (may be null): incremented once per item whose status is not 0.
// Grid: ceil(n / 16) workgroups of 64 threads; thread l works on item 16 * blockIdx.x + (l & 15) as lane q = l >> 4.
extern "C" __global__ void __launch_bounds__(64) k_schnorr_verify(const uint8_t* __restrict__ messages,
                                                                 const int* __restrict__ msg_idx,
                                                                 const int* __restrict__ key_idx,
                                                                 const uint8_t* __restrict__ sigs,
                                                                 const uint32_t* __restrict__ table, int nkeys,
                                                                 int nmsg, int n, int* __restrict__ status,
                                                                 int* counter) {
  __shared__ __align__(16) uint32_t s_part[4][SP][24];
  __shared__ uint32_t s_sc[SP][2][8];
  const int p = threadIdx.x & (SP - 1), q = threadIdx.x >> 4;
  const int t = blockIdx.x * SP + p;
  const bool valid = t < n;
  uint32_t r[8], c[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = c[i] = 0;
  int mi = -1, ki = -1;
  if (valid) {
    const uint32_t* sg = reinterpret_cast<const uint32_t*>(sigs + (long long)t * 64);
    ld_scalar_be(c, sg);
    ld_scalar_be(r, sg + 8);
    mi = msg_idx[t];
    ki = key_idx[t];
  }
  const bool in_range = valid && mi >= 0 && mi < nmsg && ki >= 0 && ki < nkeys;
  const bool below = scalar_lt_n(c) && scalar_lt_n(r);
  const bool act = in_range && below;
  partial_sums(act, r, c, ki, table, p, q, s_sc, s_part);
  // ---------------- the last barrier is behind us: one lane per item finishes
  if (!(valid && q == 0)) return;
  int st = !below ? 1 : !in_range ? 4 : 0;   // the codes' order: the range of c and r is checked first
  if (st == 0) {
    u64 key[8], msg[8], ch[4];
    marshal_sum(p, s_part, key);
    ld_words64(msg, reinterpret_cast<const uint32_t*>(messages + (long long)mi * 64));
    const int used = schnorr_challenge(key, msg, ch);
    if (used == 0) {
      st = 3;
    } else {
      u64 diff = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) diff |= ch[j] ^ (((u64)c[2 * j + 1] << 32) | c[2 * j]);
      if (diff) st = 2;
    }
  }
  status[t] = st;
  if (st != 0 && counter != nullptr) atomicAdd(counter, 1);
}

// Test entry point: the challenge alone.  tm: uint8 [n][64] marshals of T; messages: uint8 [n][64] (message i
// belongs to item i); scalar: uint8 [n][32] the challenge, big-endian (zeros at the draw cap); draws: int [n] the
// candidates drawn, 0 at the cap.
extern "C" __global__ void __launch_bounds__(64) k_schnorr_challenge(const uint8_t* __restrict__ tm,
                                                                    const uint8_t* __restrict__ messages, int n,
                                                                    uint8_t* __restrict__ scalar,
                                                                    int* __restrict__ draws) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  u64 key[8], msg[8], ch[4] = {0, 0, 0, 0};
  ld_words64(key, reinterpret_cast<const uint32_t*>(tm + (long long)t * 64));
  ld_words64(msg, reinterpret_cast<const uint32_t*>(messages + (long long)t * 64));
  const int used = schnorr_challenge(key, msg, ch);
  uint32_t* o = reinterpret_cast<uint32_t*>(scalar + (long long)t * 32);
#pragma unroll
  for (int j = 0; j < 4; ++j) {   // big-endian: limb 3 first
    const u64 be = used ? __builtin_bswap64(ch[3 - j]) : 0ull;
    o[2 * j] = (uint32_t)be;
    o[2 * j + 1] = (uint32_t)(be >> 32);
  }
  draws[t] = used;
}

// Test entry point: the point sum alone, through the verifier's own lanes.  rs, cs: uint8 [n][32] big-endian
// scalars (any 256-bit value recodes inside the table); key_idx: int [n]; out: uint8 [n][64] the marshal of
// r G + c PK (zeros for infinity and for a key index out of range).
extern "C" __global__ void __launch_bounds__(64) k_schnorr_point(const uint8_t* __restrict__ rs,
                                                                const uint8_t* __restrict__ cs,
                                                                const int* __restrict__ key_idx,
                                                                const uint32_t* __restrict__ table, int nkeys, int n,
                                                                uint8_t* __restrict__ out) {
  __shared__ __align__(16) uint32_t s_part[4][SP][24];
  __shared__ uint32_t s_sc[SP][2][8];
  const int p = threadIdx.x & (SP - 1), q = threadIdx.x >> 4;
  const int t = blockIdx.x * SP + p;
  const bool valid = t < n;
  uint32_t r[8], c[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) r[i] = c[i] = 0;
  int ki = -1;
  if (valid) {
    ld_scalar_be(r, reinterpret_cast<const uint32_t*>(rs + (long long)t * 32));
    ld_scalar_be(c, reinterpret_cast<const uint32_t*>(cs + (long long)t * 32));
    ki = key_idx[t];
  }
  const bool act = valid && ki >= 0 && ki < nkeys;
  partial_sums(act, r, c, ki, table, p, q, s_sc, s_part);
  if (!(valid && q == 0)) return;
  u64 m[8];
  marshal_sum(p, s_part, m);   // an item that took no part left four infinities: zeros
  st_words64(reinterpret_cast<uint32_t*>(out + (long long)t * 64), m);
}

// The signer (run_sign_job, schnorr_sign): item t signs message msg_idx[t] with local key key_idx[t] and nonce id
// nonce_id[t].  messages: uint8 [nmsg][64]; keys: [nkeys][8] limbs of sk 2^256 mod n; bases: uint8 [nkeys][32] the
// nonce bases; table: base 0 of a (B0 = 8, NW = 33) table, G; sigs: uint8 [n][64] (c || r, zeros unless status 0);
// status: int [n], 0 signed | 3 a XOF found no candidate in DRAWS (the host signs) | 4 an index out of range;
// counter (may be null): incremented once per item whose status is not 0.
// Grid as the verifier's.  Every lane of an item draws the nonce v itself (the wave runs the XOF once either way);
// lane q sums windows 0..8 (q = 0) or 8 q + 1 .. 8 q + 8 of v G; lane 0 adds, marshals, hashes, responds, stores.
extern "C" __global__ void __launch_bounds__(64) k_schnorr_sign(const uint8_t* __restrict__ messages,
                                                               const int* __restrict__ msg_idx,
                                                               const int* __restrict__ key_idx,
                                                               const uint32_t* __restrict__ nonce_id,
                                                               const uint32_t* __restrict__ keys,
                                                               const uint8_t* __restrict__ bases,
                                                               const uint32_t* __restrict__ table, int nkeys,
                                                               int nmsg, int n, uint8_t* __restrict__ sigs,
                                                               int* __restrict__ status, int* counter) {
  __shared__ __align__(16) uint32_t s_part[4][SP][24];
  __shared__ uint32_t s_v[SP][8];
  const int p = threadIdx.x & (SP - 1), q = threadIdx.x >> 4;
  const int t = blockIdx.x * SP + p;
  const bool valid = t < n;
  int mi = -1, ki = -1;
  uint32_t id = 0;
  if (valid) {
    mi = msg_idx[t];
    ki = key_idx[t];
    id = nonce_id[t];
  }
  const bool in_range = valid && mi >= 0 && mi < nmsg && ki >= 0 && ki < nkeys;
  u64 ent[8], v64[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 8; ++i) ent[i] = 0;
  if (in_range) ld_entropy(ent, reinterpret_cast<const uint32_t*>(bases + (long long)ki * 32), id);
  const int vdraws = schnorr_xof(XOF_KEY36, ent, false, ent, v64);   // (an item out of range draws from zeros, unused)
  const bool act = in_range && vdraws != 0;
  uint32_t v[8];
  limbs32(v, v64);
  if (q == 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) s_v[p][i] = act ? v[i] : 0u;
  }
  __syncthreads();
  jac acc = jac_inf();
  if (act) acc = window_sum(&s_v[p][0], table, q == 0 ? 0 : 8 * q + 1, q == 0 ? 9 : 8);
  st_jac(&s_part[q][p][0], acc);
  __syncthreads();
  // ---------------- the last barrier is behind us: one lane per item finishes
  if (!(valid && q == 0)) return;
  int st = !in_range ? 4 : vdraws == 0 ? 3 : 0;
  u64 out[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = 0;
  if (st == 0) {
    u64 key[8], msg[8], ch[4];
    marshal_sum(p, s_part, key);
    ld_words64(msg, reinterpret_cast<const uint32_t*>(messages + (long long)mi * 64));
    if (schnorr_challenge(key, msg, ch) == 0) {
      st = 3;
    } else {
      uint32_t c[8], skr[8], r[8];
      limbs32(c, ch);
#pragma unroll
      for (int i = 0; i < 8; ++i) skr[i] = keys[(long long)ki * 8 + i];
      schnorr_response(v, skr, c, r);
      u64 cw[4], rw[4];
      scalar_be_words(cw, c);
      scalar_be_words(rw, r);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        out[j] = cw[j];
        out[4 + j] = rw[j];
      }
    }
  }
  st_words64(reinterpret_cast<uint32_t*>(sigs + (long long)t * 64), out);
  status[t] = st;
  if (st != 0 && counter != nullptr) atomicAdd(counter, 1);
}

// Test entry point: the nonce alone.  entropy: uint8 [n][36] (a signer's base || le32(nonce id)); scalar: uint8
// [n][32] the nonce, big-endian (zeros at the draw cap); draws: int [n] the candidates drawn, 0 at the cap.
extern "C" __global__ void __launch_bounds__(64) k_schnorr_nonce(const uint8_t* __restrict__ entropy, int n,
                                                                uint8_t* __restrict__ scalar,
                                                                int* __restrict__ draws) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint32_t* e = reinterpret_cast<const uint32_t*>(entropy + (long long)t * 36);
  u64 ent[8], v[4] = {0, 0, 0, 0};
  ld_entropy(ent, e, e[8]);
  const int used = schnorr_xof(XOF_KEY36, ent, false, ent, v);
  uint32_t* o = reinterpret_cast<uint32_t*>(scalar + (long long)t * 32);
#pragma unroll
  for (int j = 0; j < 4; ++j) {   // big-endian: limb 3 first
    const u64 be = used ? __builtin_bswap64(v[3 - j]) : 0ull;
    o[2 * j] = (uint32_t)be;
    o[2 * j + 1] = (uint32_t)(be >> 32);
  }
  draws[t] = used;
}

// Test entry point: the response alone.  vs, cs: uint8 [n][32] big-endian scalars below n; skr: [n][8] limbs of
// sk 2^256 mod n; out: uint8 [n][32] v - sk c mod n, big-endian.
extern "C" __global__ void __launch_bounds__(64) k_schnorr_response(const uint8_t* __restrict__ vs,
                                                                   const uint32_t* __restrict__ skr,
                                                                   const uint8_t* __restrict__ cs, int n,
                                                                   uint8_t* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  uint32_t v[8], c[8], k[8], r[8];
  ld_scalar_be(v, reinterpret_cast<const uint32_t*>(vs + (long long)t * 32));
  ld_scalar_be(c, reinterpret_cast<const uint32_t*>(cs + (long long)t * 32));
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = skr[(long long)t * 8 + i];
  schnorr_response(v, k, c, r);
  u64 w[4];
  scalar_be_words(w, r);
  uint32_t* o = reinterpret_cast<uint32_t*>(out + (long long)t * 32);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o[2 * j] = (uint32_t)w[j];
    o[2 * j + 1] = (uint32_t)(w[j] >> 32);
  }
}

namespace {
inline bool misaligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }
}  // namespace

// -1 and no launch for n < 0, nkeys < 1, nmsg < 1, a null required pointer or a byte buffer that is not 4-byte
// aligned; 0 and no launch for n == 0.  counter may be null.
extern "C" int bsc_schnorr_verify(const uint8_t* messages, const int* msg_idx, const int* key_idx,
                                  const uint8_t* sigs, const uint32_t* table, int nkeys, int nmsg, int n, int* status,
                                  int* counter, void* stream) {
  if (n < 0 || nkeys < 1 || nmsg < 1) return -1;
  if (n == 0) return 0;
  if (!messages || !msg_idx || !key_idx || !sigs || !table || !status) return -1;
  if (misaligned4(messages) || misaligned4(sigs)) return -1;
  hipLaunchKernelGGL(k_schnorr_verify, dim3((n + SP - 1) / SP), dim3(64), 0, (hipStream_t)stream, messages, msg_idx,
                     key_idx, sigs, table, nkeys, nmsg, n, status, counter);
  return (int)hipGetLastError();
}

extern "C" int bsc_schnorr_challenge(const uint8_t* tm, const uint8_t* messages, int n, uint8_t* scalar, int* draws,
                                     void* stream) {
  if (n < 0) return -1;
  if (n == 0) return 0;
  if (!tm || !messages || !scalar || !draws) return -1;
  if (misaligned4(tm) || misaligned4(messages) || misaligned4(scalar)) return -1;
  hipLaunchKernelGGL(k_schnorr_challenge, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, tm, messages, n,
                     scalar, draws);
  return (int)hipGetLastError();
}

// The contract of bsc_schnorr_verify: -1 and no launch for n < 0, nkeys < 1, nmsg < 1, a null required pointer or a
// byte buffer that is not 4-byte aligned; 0 and no launch for n == 0.  counter may be null.
extern "C" int bsc_schnorr_sign(const uint8_t* messages, const int* msg_idx, const int* key_idx,
                                const uint32_t* nonce_id, const uint32_t* keys, const uint8_t* bases,
                                const uint32_t* table, int nkeys, int nmsg, int n, uint8_t* sigs, int* status,
                                int* counter, void* stream) {
  if (n < 0 || nkeys < 1 || nmsg < 1) return -1;
  if (n == 0) return 0;
  if (!messages || !msg_idx || !key_idx || !nonce_id || !keys || !bases || !table || !sigs || !status) return -1;
  if (misaligned4(messages) || misaligned4(bases) || misaligned4(sigs)) return -1;
  hipLaunchKernelGGL(k_schnorr_sign, dim3((n + SP - 1) / SP), dim3(64), 0, (hipStream_t)stream, messages, msg_idx,
                     key_idx, nonce_id, keys, bases, table, nkeys, nmsg, n, sigs, status, counter);
  return (int)hipGetLastError();
}

extern "C" int bsc_schnorr_nonce(const uint8_t* entropy, int n, uint8_t* scalar, int* draws, void* stream) {
  if (n < 0) return -1;
  if (n == 0) return 0;
  if (!entropy || !scalar || !draws) return -1;
  if (misaligned4(entropy) || misaligned4(scalar)) return -1;
  hipLaunchKernelGGL(k_schnorr_nonce, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, entropy, n, scalar,
                     draws);
  return (int)hipGetLastError();
}

extern "C" int bsc_schnorr_response(const uint8_t* vs, const uint32_t* skr, const uint8_t* cs, int n, uint8_t* out,
                                    void* stream) {
  if (n < 0) return -1;
  if (n == 0) return 0;
  if (!vs || !skr || !cs || !out) return -1;
  if (misaligned4(vs) || misaligned4(cs) || misaligned4(out)) return -1;
  hipLaunchKernelGGL(k_schnorr_response, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, vs, skr, cs, n, out);
  return (int)hipGetLastError();
}

extern "C" int bsc_schnorr_point(const uint8_t* rs, const uint8_t* cs, const int* key_idx, const uint32_t* table,
                                 int nkeys, int n, uint8_t* out, void* stream) {
  if (n < 0 || nkeys < 1) return -1;
  if (n == 0) return 0;
  if (!rs || !cs || !key_idx || !table || !out) return -1;
  if (misaligned4(rs) || misaligned4(cs) || misaligned4(out)) return -1;
  hipLaunchKernelGGL(k_schnorr_point, dim3((n + SP - 1) / SP), dim3(64), 0, (hipStream_t)stream, rs, cs, key_idx,
                     table, nkeys, n, out);
  return (int)hipGetLastError();
}
