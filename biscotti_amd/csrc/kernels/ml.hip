// Learning-side kernels of a Biscotti round (gfx950):
//   K1  batched softmax-regression local step: minibatch draw, (x-0.5)/0.5 transform, logits
//       (f32 MFMA), softmax + CE, backward dW (f32 MFMA) / db, clip_grad_norm(100), negate,
//       fixed-point quantisation -- one workgroup per virtual peer
//       (ML/Pytorch/client.py:38-65, client_obj.py:73-77, DistSys/kyber.go:698-710); the same body under the
//       multi-class margin loss is the SVM task's step (k_margin_step; svm_model.py, client.py:28)
//   K1m the same step of a one-hidden-layer ReLU MLP (k_mlp_step; FedSys only), K2m its evaluation (k_mlp_eval)
//   K1c the same step of the MNIST CNN, conv5x5 + ReLU + fc (k_cnn_step; FedSys only), K2c its evaluation (k_cnn_eval)
//   K1t top-k sparsification of the step's rows: per-row radix select on the fp32 magnitudes, in place
//       (ML/code/linear_model.py:48-88)
//   K3  batched logistic-regression step with DP noise at source (ML/code/logistic_model.py:92-140)
//   K4  counter-based Gaussian DP noise, averaged over each worker's noisers, added to the delta
//       (client_obj.py:42-67,97-98; DistSys/main.go:1592-1660,1530-1537)
//   K5  Multi-Krum: f64-MFMA Gram (split-K) + distances/scores/selection in LDS
//       (client_obj.py:114-143)
//   K2  test error / 1->7 attack rate (client.py:146-172)
//   K12 exact secret recovery (128-bit Newton) + dequantisation + W update (kyber.go:809-857,
//       honest.go:398-411,442-502)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "launchers.h"
#define BSC_PRIO_FLAG bsc_prio_on_ml
#include "wave_prio.h"
BSC_PRIO_SETTER(bsc_wave_prio_ml)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- Philox4x32-10
struct u4 {
  uint32_t x, y, z, w;
};
__device__ __forceinline__ u4 philox(u4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c.x;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.z;
    u4 n;
    n.x = (uint32_t)(p1 >> 32) ^ c.y ^ k0;
    n.y = (uint32_t)p1;
    n.z = (uint32_t)(p0 >> 32) ^ c.w ^ k1;
    n.w = (uint32_t)p0;
    c = n;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}
__device__ __forceinline__ float u01(uint32_t v) { return ((float)(v >> 8) + 0.5f) * (1.0f / 16777216.0f); }
__device__ __forceinline__ float gauss(uint32_t a, uint32_t b) {
  const float r = sqrtf(-2.0f * logf(u01(a)));
  return r * cosf(6.28318530717958647692f * u01(b));
}

__device__ __forceinline__ long long quantize(float v, double scale) {
  // Go: int64(float64(delta) * 10^precision) -- truncation toward zero
  return (long long)((double)v * scale);
}

}  // namespace

// =====================================================================================
// K1: softmax regression local step.  Any D_IN (K-tiled through LDS), D_OUT <= 16, B <= 16.
// X: [Ntot, D_IN] fp32 (standardised pixels), y: [Ntot] int32.  Peer p trains on rows
// [off[p], off[p] + ntrain[p]).  W: [D_OUT*D_IN + D_OUT] fp64 global model (W row-major, b).
// Outputs: delta fp32 [P, nparam], qdelta int64 [P, nparam], loss fp32 [P].
// =====================================================================================
constexpr int SM_MAXK = 1024;
constexpr int SM_THREADS = 256;

namespace {
// Step 4 of the local step, one struct per loss of the linear scorer: from one minibatch row's logits lg[0, D_OUT)
// and its label, the row of G = d(mean loss) / d(logits) (already divided by Bq) into g[0, D_OUT); returns the
// row's loss.  Everything around it (draw, transform, logits, dW / db, clip, quantisation) is linear_step_body.
struct CrossEntropyLoss {  // softmax + cross-entropy (nn.CrossEntropyLoss, client.py:29)
  static __device__ __forceinline__ float row(const float* lg, int D_OUT, int lab, int Bq, float* g) {
    float mx = -INFINITY;
    for (int c = 0; c < D_OUT; ++c) mx = fmaxf(mx, lg[c]);
    float se = 0.f;
    for (int c = 0; c < D_OUT; ++c) se += expf(lg[c] - mx);
    for (int c = 0; c < D_OUT; ++c) g[c] = (expf(lg[c] - mx) / se - (c == lab ? 1.f : 0.f)) / (float)Bq;
    return (mx + logf(se)) - lg[lab];
  }
};
// multi-class margin loss with the row's single target (SVMModel under nn.MultiLabelMarginLoss with the target
// [y, -1, ...], client.py:28 == F.multi_margin_loss(p = 1, margin = 1)): sum_{c != y} max(0, 1 - x_y + x_c) / C.
// Active where z > 0 strictly, like torch: a hinge at exactly 0 gives no gradient.
struct MarginLoss {
  static __device__ __forceinline__ float row(const float* lg, int D_OUT, int lab, int Bq, float* g) {
    const float xy = lg[lab];
    const float w = 1.f / ((float)D_OUT * (float)Bq);
    float l = 0.f;
    int act = 0;
    for (int c = 0; c < D_OUT; ++c) {
      const float z = 1.f - xy + lg[c];
      const bool on = c != lab && z > 0.f;
      g[c] = on ? w : 0.f;
      if (on) {
        l += z;
        ++act;
      }
    }
    g[lab] = -(float)act * w;
    return l / (float)D_OUT;
  }
};

template <class Loss>
__device__ __forceinline__ void linear_step_body(
    const float* X, const int* y, const long long* off, const int* ntrain, const int* pid, const double* W, int D_IN,
    int D_OUT, int B, int P, unsigned long long seed, int iteration, float max_norm, double qscale, float* delta,
    long long* qdelta, float* loss, int lo, int* ones, int nones) {
  // the next round's speculative share MSM waits for this step (and the Gram behind it on the same stream):
  // a short latency chain at the front of the round
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  // ones (optional): the next speculative MSM's row flags, set to 1 here (the MSM waits for this step anyway)
  // instead of by an upload or a kernel of their own in front of the MSM
  if (ones != nullptr && blockIdx.x == 0)
    for (int i = threadIdx.x; i < nones; i += blockDim.x) ones[i] = 1;
  __shared__ float xs[16 * SM_MAXK];  // minibatch rows, transformed; rows >= B are zero
  __shared__ float red[4][16][16];    // per-wave partial logits
  __shared__ float G[16][16];         // d(mean loss) / d(logits): (softmax - onehot) / B, or the margin's +-1 / (C B)
  __shared__ int bidx[16];
  __shared__ float nrm[SM_THREADS / 64];
  __shared__ float scale_sh;
  const int p = blockIdx.x;
  if (p >= P) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nparam = D_OUT * D_IN + D_OUT;
  // lo >= 0: off / ntrain are indexed by local peer (pid - lo), resident for every local peer, so a
  // round uploads only the peer ids; lo < 0: per-row arrays
  const int li = lo >= 0 ? pid[p] - lo : p;
  const long long offp = off[li];
  const int n = ntrain[li];
  // 1. draw B distinct minibatch indices (DataLoader(shuffle=True) takes the first batch)
  if (tid == 0) {
    int cnt = 0;
    uint32_t ctr = 0;
    while (cnt < B && cnt < n) {
      u4 r = philox(u4{(uint32_t)pid[p], (uint32_t)iteration, ctr++, 0x5EEDu}, (uint32_t)seed, (uint32_t)(seed >> 32));
      const uint32_t cand[4] = {r.x, r.y, r.z, r.w};
      for (int q = 0; q < 4 && cnt < B && cnt < n; ++q) {
        const int c = (int)(cand[q] % (uint32_t)n);
        bool dup = false;
        for (int t = 0; t < cnt; ++t) dup |= bidx[t] == c;
        if (!dup) bidx[cnt++] = c;
      }
    }
    for (int t = cnt; t < 16; ++t) bidx[t] = -1;
  }
  __syncthreads();
  const int Bq = min(B, n);
  // 2-3. logits via f32 MFMA 16x16x4: A[s][k] = xs, B[k][c] = W[c][k].  The minibatch rows are staged
  // through LDS in K tiles of SM_MAXK (one tile for MNIST's 784 features, nine for LFW's 8742);
  // within a tile the 4 waves split K, each accumulating its share across tiles in registers.
  const int ktiles = (D_IN + SM_MAXK - 1) / SM_MAXK;
  auto stage = [&](int kt) {  // (x - 0.5) / 0.5 (torchvision Normalize(0.5, 0.5)); zero padding
    const int k0 = kt * SM_MAXK, kw = min(SM_MAXK, D_IN - k0);
    for (int i = tid; i < 16 * kw; i += SM_THREADS) {
      const int s = i / kw, k = i % kw;
      float v = 0.f;
      if (s < Bq) v = (X[(offp + bidx[s]) * (long long)D_IN + k0 + k] - 0.5f) * 2.0f;
      xs[s * SM_MAXK + k] = v;
    }
  };
  {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int i = lane & 15, kk = lane >> 4;
    for (int kt = 0; kt < ktiles; ++kt) {
      const int k0 = kt * SM_MAXK, kw = min(SM_MAXK, D_IN - k0);
      if (kt > 0) __syncthreads();  // the previous tile has been consumed
      stage(kt);
      __syncthreads();
      const int ksteps = (kw + 3) / 4;
      const int per = (ksteps + 3) / 4;
      for (int st = wid * per; st < min(ksteps, (wid + 1) * per); ++st) {
        const int k = st * 4 + kk;
        const float av = (k < kw) ? xs[i * SM_MAXK + k] : 0.f;
        const float bv = (k < kw && i < D_OUT) ? (float)W[i * D_IN + k0 + k] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wid][(lane >> 4) * 4 + r][lane & 15] = acc[r];
  }
  __syncthreads();
  // 4. the loss and its gradient with respect to the logits on rows s < Bq (one thread per row)
  if (tid < 16) {
    const int s = tid;
    if (s < Bq) {
      float lg[16];
      for (int c = 0; c < D_OUT; ++c)
        lg[c] = red[0][s][c] + red[1][s][c] + red[2][s][c] + red[3][s][c] + (float)W[D_OUT * D_IN + c];
      const float l = Loss::row(lg, D_OUT, y[offp + bidx[s]], Bq, G[s]);
      for (int c = D_OUT; c < 16; ++c) G[s][c] = 0.f;
      red[0][s][0] = l;  // per-row loss (red no longer needed)
    } else {
      for (int c = 0; c < 16; ++c) G[s][c] = 0.f;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float l = 0.f;
    for (int s = 0; s < Bq; ++s) l += red[0][s][0];
    loss[p] = l / (float)max(Bq, 1);
  }
  // 5. dW[c][k] = sum_s G[s][c] xs[s][k] via f32 MFMA (M = classes, N = k tiles, K = samples); with
  // several K tiles the rows are staged again (the last tile is still resident: it goes first)
  float* dst = delta + (size_t)p * nparam;
  float sq = 0.f;
  for (int q = 0; q < ktiles; ++q) {
    const int kt = (ktiles - 1 + q) % ktiles;
    const int k0 = kt * SM_MAXK, kw = min(SM_MAXK, D_IN - k0);
    if (q > 0) {
      __syncthreads();
      stage(kt);
      __syncthreads();
    }
    const int ntiles = (kw + 15) / 16;
    const int col = lane & 15, kk = lane >> 4;
    for (int t = wid; t < ntiles; t += 4) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int s = ks * 4 + kk;
        const float av = G[s][col];  // A[c = col][s]
        const int k = t * 16 + col;
        const float bv = (k < kw) ? xs[s * SM_MAXK + k] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
      }
      const int k = t * 16 + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = (lane >> 4) * 4 + r;
        if (c < D_OUT && k < kw) {
          dst[c * D_IN + k0 + k] = acc[r];
          sq += acc[r] * acc[r];
        }
      }
    }
  }
  if (tid < D_OUT) {
    float db = 0.f;
    for (int s = 0; s < 16; ++s) db += G[s][tid];
    dst[D_OUT * D_IN + tid] = db;
    sq += db * db;
  }
  // 6. clip_grad_norm(max_norm): total L2 norm over W and b
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  if (lane == 0) nrm[wid] = sq;
  __syncthreads();
  if (tid == 0) {
    const float tot = sqrtf(nrm[0] + nrm[1] + nrm[2] + nrm[3]);
    const float coef = max_norm / (tot + 1e-6f);
    scale_sh = coef < 1.f ? coef : 1.f;
  }
  __syncthreads();
  // 7. delta = -grad (client_obj.privateFun), quantised like updateFloatToInt
  const float sc = -scale_sh;
  long long* qd = qdelta + (size_t)p * nparam;
  for (int i = tid; i < nparam; i += SM_THREADS) {
    const float v = dst[i] * sc;
    dst[i] = v;
    qd[i] = quantize(v, qscale);
  }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(SM_THREADS) k_softmax_step(
    const float* X, const int* y, const long long* off, const int* ntrain, const int* pid, const double* W, int D_IN,
    int D_OUT, int B, int P, unsigned long long seed, int iteration, float max_norm, double qscale, float* delta,
    long long* qdelta, float* loss, int lo, int* ones, int nones) {
  linear_step_body<CrossEntropyLoss>(X, y, off, ntrain, pid, W, D_IN, D_OUT, B, P, seed, iteration, max_norm, qscale,
                                     delta, qdelta, loss, lo, ones, nones);
}

// K1, margin form: the same step of the same linear scorer under the multi-class margin loss (the SVM task)
extern "C" __global__ void __launch_bounds__(SM_THREADS) k_margin_step(
    const float* X, const int* y, const long long* off, const int* ntrain, const int* pid, const double* W, int D_IN,
    int D_OUT, int B, int P, unsigned long long seed, int iteration, float max_norm, double qscale, float* delta,
    long long* qdelta, float* loss, int lo, int* ones, int nones) {
  linear_step_body<MarginLoss>(X, y, off, ntrain, pid, W, D_IN, D_OUT, B, P, seed, iteration, max_norm, qscale, delta,
                               qdelta, loss, lo, ones, nones);
}

// =====================================================================================
// K1m: local step of a one-hidden-layer MLP, x -> h = relu(W1 x + b1) -> logits = W2 h + b2, under cross-entropy.
// H = 16 NCT hidden units (NCT = 1..4 column tiles of 16), D_OUT <= 16, B <= 16, any D_IN.  W fp64, flat in torch's
// parameters() order: [W1 (H x D_IN, row-major) | b1 (H) | W2 (D_OUT x H, row-major) | b2 (D_OUT)].  The minibatch
// draw, the transform, a shard shorter than B, the clip of the whole gradient, delta = -clipped gradient, the
// quantisation and the per-peer loss are K1's.  One 256-thread workgroup per peer, the batch one 16-row MFMA tile:
//   forward  Z1 = X W1^T on f32 MFMA 16x16x4, X staged MLP_KT features at a time (rows MLP_KS floats apart: the 16
//            rows of an A operand fall into 16 different bank groups).  Within a tile the 4 waves split K and every
//            wave feeds all NCT column tiles from one A operand read (a split by column tile would leave three waves
//            idle at H = 16); the accumulators stay in registers across the tiles.  The same A register as A and B
//            gives the Gram X X^T of the minibatch rows: one more MFMA per k step, no more LDS reads
//   middle   h = relu(Z1 + b1), logits (K = H, wave 0), the loss rows (K1's CrossEntropyLoss), dW2 = G^T h and
//            dH = (G W2) masked by h > 0 (column tile j on wave j), db1, db2: all in LDS and registers; the raw small
//            gradient [db1 | dW2 | db2] waits in LDS for the clip
//   clip     ||dW1||_F^2 = sum_st (dH dH^T)_st (X X^T)_st, one (s, t) term per thread, combined in fp64 in a fixed
//            order with the small part's squares: the coefficient is known before dW1 exists
//   dW1      = dH^T X (M = hidden units, N = k tile, K = samples): the tiles of X are staged again (the last one is
//            still resident: it goes first), each output entry is scaled, quantised and stored once by the lane
//            that finished it.  No H x D_IN accumulator lives across a barrier and delta is written once
// LDS, all static (bytes): 17664 tile + 4096 NCT forward partials + 4096 Gram partials + 192 (H + 1) of h, dH, W2
// + 68 H + 64 small gradient + 2048 logits and G + 296 = 32616 / 40872 / 49128 / 57384 at H = 16 / 32 / 48 / 64
// (the compiler's figures): inside the default 64 KiB, no attribute is set at launch.
// No atomics, no reduction whose order depends on timing: two runs give the same bytes.
// =====================================================================================
constexpr int MLP_KT = 256;          // == the block: one thread per staged column
constexpr int MLP_KS = MLP_KT + 20;

namespace {
// rows rowidx[0, 16) of X (< 0: a zero row), features [k0, k0 + kw), as (x - tsub) * tmul
__device__ __forceinline__ void mlp_stage(float* xs, const float* X, const long long* rowidx, int D_IN, int k0, int kw,
                                          float tsub, float tmul) {
  const int k = threadIdx.x;
  if (k < kw) {
#pragma unroll 4
    for (int s = 0; s < 16; ++s) {
      const long long r = rowidx[s];
      xs[s * MLP_KS + k] = r >= 0 ? (X[r * (long long)D_IN + k0 + k] - tsub) * tmul : 0.f;
    }
  }
}

// the staged tile's share of Z1 = X W1^T (and of X X^T), this wave's quarter of the tile's k steps
template <int NCT, bool GRAM>
__device__ __forceinline__ void mlp_hidden_tile(const float* xs, const double* W1, int D_IN, int k0, int kw,
                                                f32x4 (&acc)[NCT], f32x4& accg) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, i = lane & 15, kk = lane >> 4;
  const int ksteps = (kw + 3) / 4, per = (ksteps + 3) / 4;
  const int st1 = min(ksteps, (wid + 1) * per);
#pragma unroll 2
  for (int st = wid * per; st < st1; ++st) {
    const int k = st * 4 + kk;
    const bool in = k < kw;
    const float av = in ? xs[i * MLP_KS + k] : 0.f;
    float bv[NCT];
#pragma unroll
    for (int j = 0; j < NCT; ++j) bv[j] = in ? (float)W1[(size_t)(j * 16 + i) * D_IN + k0 + k] : 0.f;
#pragma unroll
    for (int j = 0; j < NCT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[j], acc[j], 0, 0, 0);
    if (GRAM) accg = __builtin_amdgcn_mfma_f32_16x16x4f32(av, av, accg, 0, 0, 0);
  }
}

// Z1 over every tile of D_IN as four per-wave partials in red (and the Gram's in redg); the last tile stays in xs
template <int NCT, bool GRAM>
__device__ __forceinline__ void mlp_hidden_partials(float* xs, float (&red)[4][NCT][16][16], float (*redg)[16][16],
                                                    const float* X, const long long* rowidx, const double* W1,
                                                    int D_IN, float tsub, float tmul) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  f32x4 acc[NCT], accg = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NCT; ++j) acc[j] = accg;
  const int ktiles = (D_IN + MLP_KT - 1) / MLP_KT;
  for (int kt = 0; kt < ktiles; ++kt) {
    const int k0 = kt * MLP_KT, kw = min(MLP_KT, D_IN - k0);
    if (kt > 0) __syncthreads();  // the previous tile has been consumed
    mlp_stage(xs, X, rowidx, D_IN, k0, kw, tsub, tmul);
    __syncthreads();
    mlp_hidden_tile<NCT, GRAM>(xs, W1, D_IN, k0, kw, acc, accg);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int j = 0; j < NCT; ++j) red[wid][j][(lane >> 4) * 4 + r][lane & 15] = acc[j][r];
    if (GRAM) redg[wid][(lane >> 4) * 4 + r][lane & 15] = accg[r];
  }
  __syncthreads();
}

// h[s][u] = relu(Z1[s][u] + b1[u]) on rows s < rows, 0 on the others
template <int NCT>
__device__ __forceinline__ void mlp_hidden_relu(const float (&red)[4][NCT][16][16], const double* b1, int rows,
                                                float (&hs)[16][NCT * 16 + 1]) {
  constexpr int H = NCT * 16;
  for (int e = threadIdx.x; e < 16 * H; e += 256) {
    const int s = e / H, u = e % H, j = u >> 4, c = u & 15;
    const float z = (red[0][j][s][c] + red[1][j][s][c]) + (red[2][j][s][c] + red[3][j][s][c]) + (float)b1[u];
    hs[s][u] = (s < rows && z > 0.f) ? z : 0.f;
  }
  __syncthreads();
}
}  // namespace

template <int NCT>
__global__ void __launch_bounds__(256) k_mlp_step(const float* X, const int* y, const long long* off, const int* ntrain,
                                                  const int* pid, const double* W, int D_IN, int D_OUT, int B, int P,
                                                  unsigned long long seed, int iteration, float max_norm, double qscale,
                                                  float* delta, long long* qdelta, float* loss, int lo) {
  constexpr int H = NCT * 16;
  __shared__ float xs[16 * MLP_KS];     // minibatch rows, transformed; rows >= Bq are zero
  __shared__ float red[4][NCT][16][16];  // per-wave partials of Z1
  __shared__ float redg[4][16][16];     // per-wave partials of X X^T
  __shared__ float hs[16][H + 1];       // relu(Z1 + b1)
  __shared__ float dh[16][H + 1];       // d(mean loss) / d(Z1)
  __shared__ float w2s[16][H + 1];      // (float)W2, rows >= D_OUT zero
  __shared__ float lg[16][16];
  __shared__ float G[16][16];           // d(mean loss) / d(logits)
  __shared__ float gs[H + 16 * H + 16];  // the raw [db1 | dW2 | db2]
  __shared__ float rowloss[16];
  __shared__ long long rowidx[16];
  __shared__ int bidx[16];
  __shared__ double nrm[4];
  __shared__ float scale_sh;
  const int p = blockIdx.x;
  if (p >= P) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, kk = lane >> 4;
  const double *b1 = W + (size_t)H * D_IN, *W2 = b1 + H, *b2 = W2 + D_OUT * H;
  const int nsmall = H + D_OUT * H + D_OUT;
  const size_t nparam = (size_t)H * D_IN + nsmall;
  const int li = lo >= 0 ? pid[p] - lo : p;
  const long long offp = off[li];
  const int n = ntrain[li];
  // 1. K1's draw: B distinct minibatch indices from the same Philox counters
  if (tid == 0) {
    int cnt = 0;
    uint32_t ctr = 0;
    while (cnt < B && cnt < n) {
      u4 r = philox(u4{(uint32_t)pid[p], (uint32_t)iteration, ctr++, 0x5EEDu}, (uint32_t)seed, (uint32_t)(seed >> 32));
      const uint32_t cand[4] = {r.x, r.y, r.z, r.w};
      for (int q = 0; q < 4 && cnt < B && cnt < n; ++q) {
        const int c = (int)(cand[q] % (uint32_t)n);
        bool dup = false;
        for (int t = 0; t < cnt; ++t) dup |= bidx[t] == c;
        if (!dup) bidx[cnt++] = c;
      }
    }
    for (int t = 0; t < 16; ++t) rowidx[t] = t < cnt ? offp + bidx[t] : -1;
  }
  for (int e = tid; e < 16 * H; e += 256) w2s[e / H][e % H] = e / H < D_OUT ? (float)W2[e] : 0.f;
  __syncthreads();
  const int Bq = min(B, n);
  // 2. forward: Z1 (+ the Gram of the rows), h
  mlp_hidden_partials<NCT, true>(xs, red, redg, X, rowidx, W, D_IN, 0.5f, 2.0f);
  mlp_hidden_relu<NCT>(red, b1, Bq, hs);
  // 3. logits = h W2^T (wave 0; b2 joins in the loss rows)
  if (wid == 0) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < H / 4; ++st)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hs[i][st * 4 + kk], w2s[i][st * 4 + kk], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) lg[kk * 4 + r][i] = acc[r];
  }
  __syncthreads();
  // 4. the loss and its gradient with respect to the logits on rows s < Bq (one thread per row)
  if (tid < 16) {
    const int s = tid;
    float l = 0.f;
    if (s < Bq) {
      float lr[16];
      for (int c = 0; c < D_OUT; ++c) lr[c] = lg[s][c] + (float)b2[c];
      l = CrossEntropyLoss::row(lr, D_OUT, y[rowidx[s]], Bq, G[s]);
      for (int c = D_OUT; c < 16; ++c) G[s][c] = 0.f;
    } else {
      for (int c = 0; c < 16; ++c) G[s][c] = 0.f;
    }
    rowloss[s] = l;
  }
  __syncthreads();
  if (tid == 0) {
    float l = 0.f;
    for (int s = 0; s < Bq; ++s) l += rowloss[s];
    loss[p] = l / (float)max(Bq, 1);
  }
  // 5. column tile j on wave j: dW2[c][u] = sum_s G[s][c] h[s][u] (M = classes, K = samples) and
  // dH[s][u] = sum_c G[s][c] W2[c][u] where h[s][u] > 0 (M = samples, K = classes)
  for (int j = wid; j < NCT; j += 4) {
    f32x4 accw = {0.f, 0.f, 0.f, 0.f}, acch = {0.f, 0.f, 0.f, 0.f};
    const int u = j * 16 + i;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int q = ks * 4 + kk;
      accw = __builtin_amdgcn_mfma_f32_16x16x4f32(G[q][i], hs[q][u], accw, 0, 0, 0);
      acch = __builtin_amdgcn_mfma_f32_16x16x4f32(G[i][q], w2s[q][u], acch, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = kk * 4 + r;   // the class of accw's row, the sample of acch's
      if (q < D_OUT) gs[H + q * H + u] = accw[r];
      dh[q][u] = hs[q][u] > 0.f ? acch[r] : 0.f;
    }
  }
  if (tid < D_OUT) {
    float db = 0.f;
    for (int s = 0; s < 16; ++s) db += G[s][tid];
    gs[H + D_OUT * H + tid] = db;
  }
  __syncthreads();
  if (tid < H) {
    float db = 0.f;
    for (int s = 0; s < 16; ++s) db += dh[s][tid];
    gs[tid] = db;
  }
  // 6. clip_grad_norm(max_norm) over all four parameter blocks, before dW1 exists
  double part;
  {
    const int s = tid >> 4, t = tid & 15;
    float dd = 0.f;
    for (int u = 0; u < H; ++u) dd += dh[s][u] * dh[t][u];
    const float xx = (redg[0][s][t] + redg[1][s][t]) + (redg[2][s][t] + redg[3][s][t]);
    part = (double)dd * (double)xx;
  }
  __syncthreads();
  for (int e = tid; e < nsmall; e += 256) part += (double)gs[e] * (double)gs[e];
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) nrm[wid] = part;
  __syncthreads();
  if (tid == 0) {
    const float tot = sqrtf((float)fmax((nrm[0] + nrm[1]) + (nrm[2] + nrm[3]), 0.0));
    const float coef = max_norm / (tot + 1e-6f);
    scale_sh = coef < 1.f ? coef : 1.f;
  }
  __syncthreads();
  // 7. delta = -clipped gradient, quantised like updateFloatToInt: the small blocks, then dW1 tile by tile
  const float sc = -scale_sh;
  float* dst = delta + (size_t)p * nparam;
  long long* qd = qdelta + (size_t)p * nparam;
  for (int e = tid; e < nsmall; e += 256) {
    const float v = gs[e] * sc;
    dst[(size_t)H * D_IN + e] = v;
    qd[(size_t)H * D_IN + e] = quantize(v, qscale);
  }
  float ah[NCT][4];   // A[u][s] of dW1 = dH^T X, every column tile
#pragma unroll
  for (int j = 0; j < NCT; ++j)
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) ah[j][ks] = dh[ks * 4 + kk][j * 16 + i];
  const int ktiles = (D_IN + MLP_KT - 1) / MLP_KT;
  for (int q = 0; q < ktiles; ++q) {
    const int kt = (ktiles - 1 + q) % ktiles;
    const int k0 = kt * MLP_KT, kw = min(MLP_KT, D_IN - k0);
    if (q > 0) {
      __syncthreads();
      mlp_stage(xs, X, rowidx, D_IN, k0, kw, 0.5f, 2.0f);
      __syncthreads();
    }
    const int ntiles = (kw + 15) / 16;
    for (int t = wid; t < ntiles; t += 4) {
      const int k = t * 16 + i;
      const bool in = k < kw;
      float bx[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) bx[ks] = in ? xs[(ks * 4 + kk) * MLP_KS + k] : 0.f;
#pragma unroll
      for (int j = 0; j < NCT; ++j) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ah[j][ks], bx[ks], acc, 0, 0, 0);
        if (in) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const size_t e = (size_t)(j * 16 + kk * 4 + r) * D_IN + k0 + k;
            const float v = acc[r] * sc;
            dst[e] = v;
            qd[e] = quantize(v, qscale);
          }
        }
      }
    }
  }
}

// =====================================================================================
// K1c: local step of the MNIST CNN (mnist_cnn_model.py): x (S x S, S <= 28) -> z = conv5x5(x, padding 4) + bc, 16
// channels on Q x Q positions (Q = S + 4, NP = Q^2 <= 1024) -> a = relu(z) -> logits = Wfc a + bfc, under
// cross-entropy.  D_OUT <= 16, B <= 16.  W fp64, flat in torch's parameters() order: [conv.weight (16 x 25) |
// conv.bias (16) | fc.weight (D_OUT x F, F = 16 NP, feature c NP + oy Q + ox) | fc.bias (D_OUT)].  The draw, the
// transform, a shard shorter than B, the clip of the whole gradient, the quantisation and the loss are K1's;
// delta = -lr * clipped gradient.  One 256-thread workgroup per peer; the 1 MB activation map never exists: it is
// recomputed per position in each of the three passes from the images in LDS.
//   images   the minibatch's 16 images are staged once, transformed, rows >= Bq zero, one image IS = S^2 | 1 floats
//            apart (odd: the 16 samples of an operand fall into 16 banks); X is not read again
//   tile     one output position, all 16 samples and 16 channels: f32 MFMA 16x16x4 over K = the 25 taps padded to 28
//            (7 k steps).  The lane (i, kk) holds conv.weight[channel i][tap 4 st + kk] in registers for the whole
//            kernel and gathers pixel (sample i, tap 4 st + kk) from LDS, 0 outside the image (the zero padding).
//            Weights as A and pixels as B give z[channel 4 kk + r][sample i]; swapped they give
//            z[sample 4 kk + r][channel i]: the same registers, either layout
//   k order  an accumulator register is used as the next MFMA's operand without a transpose: k step r of the next
//            product takes k = (kk; r), i.e. index 4 kk + r, and the other operand is loaded in that order
//   forward  channel-major tiles: logits^T += Wfc[:, tile] a (K = channels) and the Gram A A^T += a^T a of the
//            samples' activations, from the same registers
//   middle   the loss rows (K1's CrossEntropyLoss), G, dbfc, and the fc block's share of the squared norm,
//            sum_st (G G^T)_st (A A^T)_st, one term per thread
//   conv     sample-major tiles: dA = G Wfc[:, tile] masked by a > 0, dbc, and dWconv^T += patch^T dA (M = taps in
//            two tiles of 16, N = channels, K = samples), per-wave accumulators reduced once
//   clip     the three small blocks' squares join the fc term in fp64, fixed order: the coefficient is known before
//            dWfc exists
//   write    sample-major tiles a third time: dWfc[:, tile] = G^T a (K = samples), scaled by -lr * coef into the
//            wave's stage buffer; after 16 positions the buffer's rows (class, channel) leave as 16 consecutive
//            entries each: delta and qdelta are written once, in 64 B / 128 B pieces
//   Wfc      the same stage buffer brings Wfc in for the forward and conv passes: per block of 16 positions each
//            (class, channel) row is read as one 128 B line of fp64 and kept as fp32
// The waves deal the blocks of 16 positions round-robin (block b on wave b & 3; all waves run the same number of
// iterations, so the barriers are uniform); per-wave partials are combined as (0 + 1) + (2 + 3).
// LDS (bytes): dynamic 16 * 785 * 4 = 50240 of images + 4 * 256 * 17 * 4 = 69632 of stage buffers (rows 17 floats
// apart) = 119872; static 8192 partials + 256 bias partials + 1024 G + 1728 small gradient + 296 = 11496 (the
// compiler's figure is in docs/PERF.md).  131368 in all: past the default 64 KiB, inside gfx950's 160 KiB; the
// launcher raises the dynamic limit once (hipFuncSetAttribute).
// No atomics, no reduction whose order depends on timing: two runs give the same bytes.
// =====================================================================================
constexpr int CNN_SMAX = 28;
constexpr int CNN_IMG = 16 * (CNN_SMAX * CNN_SMAX + 1);   // floats of the image area
constexpr int CNN_TS = 17;                                // floats between two rows of a stage buffer
constexpr int CNN_STAGE = 256 * CNN_TS;                   // floats of one wave's stage buffer
constexpr int CNN_DYN_LDS = (CNN_IMG + 4 * CNN_STAGE) * (int)sizeof(float);

namespace {
struct CnnLane {   // what lane (i, kk) keeps for the whole kernel, per k step st: tap t = 4 st + kk
  float w[7];      // conv.weight[channel i][t], 0 past tap 24
  int dy[7], dx[7];  // the tap's offset from the output position into the unpadded image; far outside past tap 24
};

__device__ __forceinline__ CnnLane cnn_lane(const double* Wc) {
  const int lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
  CnnLane L;
#pragma unroll
  for (int st = 0; st < 7; ++st) {
    const int t = st * 4 + kk;
    L.w[st] = t < 25 ? (float)Wc[i * 25 + t] : 0.f;
    L.dy[st] = t < 25 ? t / 5 - 4 : -64;
    L.dx[st] = t % 5 - 4;
  }
  return L;
}

// pixel (iy, ix) of the image at im, 0 outside it; the address stays inside the image either way
__device__ __forceinline__ float cnn_px(const float* im, int S, int iy, int ix) {
  const bool in = (unsigned)iy < (unsigned)S && (unsigned)ix < (unsigned)S;
  const float v = im[in ? iy * S + ix : 0];
  return in ? v : 0.f;
}

// rows rowidx[0, 16) of X (< 0: a zero image) as (x - tsub) * tmul, image s at img + s * IS
__device__ __forceinline__ void cnn_stage_images(float* img, const float* X, const long long* rowidx, int S, int IS,
                                                 float tsub, float tmul) {
  const int d_in = S * S;
  for (int e = threadIdx.x; e < 16 * d_in; e += 256) {
    const int s = e / d_in, k = e - s * d_in;
    const long long r = rowidx[s];
    img[s * IS + k] = r >= 0 ? (X[r * (long long)d_in + k] - tsub) * tmul : 0.f;
  }
}

// the pre-activations of position (oy, ox) without the bias.  SAMPLES_M: z[sample 4 kk + r][channel i], else
// z[channel 4 kk + r][sample i].  im: the image of sample i
template <bool SAMPLES_M>
__device__ __forceinline__ f32x4 cnn_conv_tile(const float* im, int S, int oy, int ox, const CnnLane& L) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < 7; ++st) {
    const float pv = cnn_px(im, S, oy + L.dy[st], ox + L.dx[st]);
    acc = SAMPLES_M ? __builtin_amdgcn_mfma_f32_16x16x4f32(pv, L.w[st], acc, 0, 0, 0)
                    : __builtin_amdgcn_mfma_f32_16x16x4f32(L.w[st], pv, acc, 0, 0, 0);
  }
  return acc;
}

// Wfc[class][c NP + pos0 + p], p < bw <= 16, into this wave's stage buffer as fp32: row class * 16 + c
// (CLASS_MAJOR) or c * 16 + class, p along the row.  A (class, c) row is 16 lanes' consecutive fp64
template <bool CLASS_MAJOR>
__device__ __forceinline__ void cnn_stage_wfc(float* stg, const double* Wfc, int NP, int D_OUT, int pos0, int bw) {
  const int lane = threadIdx.x & 63, p = lane & 15;
  for (int q = lane >> 4; q < 16 * D_OUT; q += 4) {
    const int cls = q >> 4, c = q & 15;
    if (p < bw)
      stg[(CLASS_MAJOR ? q : c * 16 + cls) * CNN_TS + p] = (float)Wfc[((size_t)cls * 16 + c) * NP + pos0 + p];
  }
}

// The forward pass over every position: this wave's partial logits^T (accl[r] = [class 4 kk + r][sample i]) and,
// with GRAM, its partial A A^T (accg[r] = [sample 4 kk + r][sample i]).  rows: samples >= rows count as absent
template <bool GRAM>
__device__ __forceinline__ void cnn_forward(const float* img, float* stg, int S, const double* Wfc, const double* bc,
                                            int D_OUT, int rows, const CnnLane& L, f32x4& accl, f32x4& accg) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, i = lane & 15, kk = lane >> 4;
  const int Q = S + 4, NP = Q * Q, IS = (S * S) | 1;
  const int iters = ((NP + 15) / 16 + 3) / 4;
  const float* im = img + i * IS;
  float bcq[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) bcq[r] = (float)bc[kk * 4 + r];
  for (int it = 0; it < iters; ++it) {
    const int pos0 = (it * 4 + wid) * 16, bw = min(16, NP - pos0);   // bw <= 0: no block left for this wave
    cnn_stage_wfc<false>(stg, Wfc, NP, D_OUT, pos0, bw);
    __syncthreads();
    for (int p = 0; p < bw; ++p) {
      const int pos = pos0 + p, oy = pos / Q, ox = pos - oy * Q;
      const f32x4 z = cnn_conv_tile<false>(im, S, oy, ox, L);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = z[r] + bcq[r];
        const float a = (i < rows && v > 0.f) ? v : 0.f;                                  // [channel 4 kk + r][sample i]
        const float wf = i < D_OUT ? stg[((kk * 4 + r) * 16 + i) * CNN_TS + p] : 0.f;     // Wfc[class i][that channel]
        accl = __builtin_amdgcn_mfma_f32_16x16x4f32(wf, a, accl, 0, 0, 0);
        if (GRAM) accg = __builtin_amdgcn_mfma_f32_16x16x4f32(a, a, accg, 0, 0, 0);
      }
    }
    __syncthreads();   // the block has been consumed: the buffer may be filled again
  }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_cnn_step(const float* X, const int* y, const long long* off,
                                                             const int* ntrain, const int* pid, const double* W, int S,
                                                             int D_OUT, int B, int P, unsigned long long seed,
                                                             int iteration, float max_norm, double qscale, float lr,
                                                             float* delta, long long* qdelta, float* loss, int lo) {
  extern __shared__ float cnn_lds[];    // images [16][IS], then one stage buffer per wave
  __shared__ float red[4][2][16][16];   // per-wave partials: logits^T and A A^T, later the two tap tiles of dWconv^T
  __shared__ float redb[4][16];         // per-wave partials of dbc
  __shared__ float G[16][16];           // d(mean loss) / d(logits)
  __shared__ float gs[416 + 16];        // the raw [dWconv | dbc | dbfc]
  __shared__ float rowloss[16];
  __shared__ long long rowidx[16];
  __shared__ int bidx[16];
  __shared__ double nrm[4];
  __shared__ float scale_sh;
  const int p = blockIdx.x;
  if (p >= P) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, kk = lane >> 4;
  const int Q = S + 4, NP = Q * Q, IS = (S * S) | 1, F = 16 * NP;
  const double *bc = W + 400, *Wfc = W + 416, *bfc = Wfc + (size_t)D_OUT * F;
  const size_t nparam = 416 + (size_t)D_OUT * F + D_OUT;
  float* img = cnn_lds;
  float* stg = cnn_lds + CNN_IMG + wid * CNN_STAGE;
  const int li = lo >= 0 ? pid[p] - lo : p;
  const long long offp = off[li];
  const int n = ntrain[li];
  // 1. K1's draw: B distinct minibatch indices from the same Philox counters
  if (tid == 0) {
    int cnt = 0;
    uint32_t ctr = 0;
    while (cnt < B && cnt < n) {
      u4 r = philox(u4{(uint32_t)pid[p], (uint32_t)iteration, ctr++, 0x5EEDu}, (uint32_t)seed, (uint32_t)(seed >> 32));
      const uint32_t cand[4] = {r.x, r.y, r.z, r.w};
      for (int q = 0; q < 4 && cnt < B && cnt < n; ++q) {
        const int c = (int)(cand[q] % (uint32_t)n);
        bool dup = false;
        for (int t = 0; t < cnt; ++t) dup |= bidx[t] == c;
        if (!dup) bidx[cnt++] = c;
      }
    }
    for (int t = 0; t < 16; ++t) rowidx[t] = t < cnt ? offp + bidx[t] : -1;
  }
  __syncthreads();
  const int Bq = min(B, n);
  cnn_stage_images(img, X, rowidx, S, IS, 0.5f, 2.0f);
  const CnnLane L = cnn_lane(W);
  __syncthreads();
  // 2. forward: the logits and the Gram of the activations, per wave, then in LDS
  {
    f32x4 accl = {0.f, 0.f, 0.f, 0.f}, accg = {0.f, 0.f, 0.f, 0.f};
    cnn_forward<true>(img, stg, S, Wfc, bc, D_OUT, Bq, L, accl, accg);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      red[wid][0][kk * 4 + r][i] = accl[r];
      red[wid][1][kk * 4 + r][i] = accg[r];
    }
  }
  __syncthreads();
  // 3. the loss and its gradient with respect to the logits on rows s < Bq (one thread per row)
  if (tid < 16) {
    const int s = tid;
    float l = 0.f;
    if (s < Bq) {
      float lr_[16];
      for (int c = 0; c < D_OUT; ++c)
        lr_[c] = (red[0][0][c][s] + red[1][0][c][s]) + (red[2][0][c][s] + red[3][0][c][s]) + (float)bfc[c];
      l = CrossEntropyLoss::row(lr_, D_OUT, y[rowidx[s]], Bq, G[s]);
      for (int c = D_OUT; c < 16; ++c) G[s][c] = 0.f;
    } else {
      for (int c = 0; c < 16; ++c) G[s][c] = 0.f;
    }
    rowloss[s] = l;
  }
  __syncthreads();
  if (tid == 0) {
    float l = 0.f;
    for (int s = 0; s < Bq; ++s) l += rowloss[s];
    loss[p] = l / (float)max(Bq, 1);
  }
  if (tid < D_OUT) {
    float db = 0.f;
    for (int s = 0; s < 16; ++s) db += G[s][tid];
    gs[416 + tid] = db;
  }
  // the fc block's share of the squared norm: ||G^T A||_F^2 = sum_st (G G^T)_st (A A^T)_st, one term per thread
  double part;
  {
    const int s = tid >> 4, t = tid & 15;
    float gg = 0.f;
    for (int c = 0; c < 16; ++c) gg += G[s][c] * G[t][c];
    const float aa = (red[0][1][s][t] + red[1][1][s][t]) + (red[2][1][s][t] + red[3][1][s][t]);
    part = (double)gg * (double)aa;
  }
  __syncthreads();   // red is free again
  // 4. the conv gradient: sample-major tiles, dA = G Wfc masked by a > 0, dbc and dWconv^T = patch^T dA
  {
    float ga[4];   // G[sample i][class 4 st + kk]
#pragma unroll
    for (int st = 0; st < 4; ++st) ga[st] = G[i][st * 4 + kk];
    const float bci = (float)bc[i];
    const int t1 = 16 + i;   // the second tap tile's tap of this lane (as A's row)
    const int dy0 = i / 5 - 4, dx0 = i % 5 - 4, dy1 = t1 < 25 ? t1 / 5 - 4 : -64, dx1 = t1 % 5 - 4;
    const float* im = img + i * IS;
    f32x4 aw0 = {0.f, 0.f, 0.f, 0.f}, aw1 = {0.f, 0.f, 0.f, 0.f};
    float dbs = 0.f;
    const int iters = ((NP + 15) / 16 + 3) / 4;
    for (int it = 0; it < iters; ++it) {
      const int pos0 = (it * 4 + wid) * 16, bw = min(16, NP - pos0);
      cnn_stage_wfc<true>(stg, Wfc, NP, D_OUT, pos0, bw);
      __syncthreads();
      for (int q = 0; q < bw; ++q) {
        const int pos = pos0 + q, oy = pos / Q, ox = pos - oy * Q;
        const f32x4 z = cnn_conv_tile<true>(im, S, oy, ox, L);
        f32x4 da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < 4; ++st) {
          const int cls = st * 4 + kk;
          const float wf = cls < D_OUT ? stg[(cls * 16 + i) * CNN_TS + q] : 0.f;   // Wfc[class][channel i]
          da = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[st], wf, da, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int s = kk * 4 + r;
          const float dz = (s < Bq && z[r] + bci > 0.f) ? da[r] : 0.f;   // [sample 4 kk + r][channel i]
          dbs += dz;
          const float* ims = img + s * IS;
          aw0 = __builtin_amdgcn_mfma_f32_16x16x4f32(cnn_px(ims, S, oy + dy0, ox + dx0), dz, aw0, 0, 0, 0);
          aw1 = __builtin_amdgcn_mfma_f32_16x16x4f32(cnn_px(ims, S, oy + dy1, ox + dx1), dz, aw1, 0, 0, 0);
        }
      }
      __syncthreads();
    }
    dbs += __shfl_xor(dbs, 16);
    dbs += __shfl_xor(dbs, 32);
    if (kk == 0) redb[wid][i] = dbs;
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // [tap 4 kk + r (+ 16)][channel i]
      red[wid][0][kk * 4 + r][i] = aw0[r];
      red[wid][1][kk * 4 + r][i] = aw1[r];
    }
  }
  __syncthreads();
  for (int e = tid; e < 416; e += 256) {
    if (e < 400) {
      const int ch = e / 25, t = e - ch * 25, h = t >> 4, tt = t & 15;
      gs[e] = (red[0][h][tt][ch] + red[1][h][tt][ch]) + (red[2][h][tt][ch] + red[3][h][tt][ch]);
    } else {
      gs[e] = (redb[0][e - 400] + redb[1][e - 400]) + (redb[2][e - 400] + redb[3][e - 400]);
    }
  }
  __syncthreads();
  // 5. clip_grad_norm(max_norm) over all four parameter blocks, before dWfc exists
  for (int e = tid; e < 416 + D_OUT; e += 256) part += (double)gs[e] * (double)gs[e];
  for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
  if (lane == 0) nrm[wid] = part;
  __syncthreads();
  if (tid == 0) {
    const float tot = sqrtf((float)fmax((nrm[0] + nrm[1]) + (nrm[2] + nrm[3]), 0.0));
    const float coef = max_norm / (tot + 1e-6f);
    scale_sh = coef < 1.f ? coef : 1.f;
  }
  __syncthreads();
  // 6. delta = -lr * clipped gradient, quantised like updateFloatToInt: the small blocks, then dWfc block by block
  const float sc = -lr * scale_sh;
  float* dst = delta + (size_t)p * nparam;
  long long* qd = qdelta + (size_t)p * nparam;
  for (int e = tid; e < 416 + D_OUT; e += 256) {
    const float v = gs[e] * sc;
    const size_t at = e < 416 ? (size_t)e : 416 + (size_t)D_OUT * F + (e - 416);
    dst[at] = v;
    qd[at] = quantize(v, qscale);
  }
  {
    float gw[4];   // G[sample 4 kk + r][class i]
#pragma unroll
    for (int r = 0; r < 4; ++r) gw[r] = G[kk * 4 + r][i];
    const float bci = (float)bc[i];
    const float* im = img + i * IS;
    const int iters = ((NP + 15) / 16 + 3) / 4;
    for (int it = 0; it < iters; ++it) {
      const int pos0 = (it * 4 + wid) * 16, bw = min(16, NP - pos0);
      for (int q = 0; q < bw; ++q) {
        const int pos = pos0 + q, oy = pos / Q, ox = pos - oy * Q;
        const f32x4 z = cnn_conv_tile<true>(im, S, oy, ox, L);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v = z[r] + bci;
          const float a = (kk * 4 + r < Bq && v > 0.f) ? v : 0.f;   // [sample 4 kk + r][channel i]
          o = __builtin_amdgcn_mfma_f32_16x16x4f32(gw[r], a, o, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) stg[((kk * 4 + r) * 16 + i) * CNN_TS + q] = o[r] * sc;   // [class 4 kk + r][channel i]
      }
      __syncthreads();
      const int pp = lane & 15;
      if (pp < bw) {
        for (int q = lane >> 4; q < 16 * D_OUT; q += 4) {   // row q = (class, channel): 16 consecutive entries
          const size_t at = 416 + (size_t)q * NP + pos0 + pp;
          const float v = stg[q * CNN_TS + pp];
          dst[at] = v;
          qd[at] = quantize(v, qscale);
        }
      }
      __syncthreads();
    }
  }
}

// =====================================================================================
// K1e: E local SGD steps of the same linear scorer per round (FedAvg-style local work, --local-steps E).
//   a_0 = 0;  step e: w_e = (float)W + a_e, minibatch e (Philox tag 0x5EED ^ (e << 16): step 0 draws K1's rows),
//   g_e = d(mean loss)/dw at w_e, c_e = min(1, max_norm / (||g_e|| + 1e-6)), a_{e+1} = a_e - lr c_e g_e;
//   delta = a_E (not clipped again), qdelta = quantize(delta), loss = the last step's mean row loss.
// One 256-thread workgroup per peer; what differs from K1:
//   a       the accumulated update stays resident for all E steps: in LDS when nparam <= LS_LDS_A (mnist: 7850
//           floats), else in the peer's own delta row, which no other workgroup touches and which stays L2-hot
//           (A_IN_LDS = false; lfw: 17486 floats)
//   draws   lane e of wave 0 draws step e's minibatch, all E draws at once in front of step 0 (E <= 64)
//   tile    the minibatch rows are staged LS_KT = 256 features at a time, rows LS_KS = LS_KT + 20 floats apart: the
//           16 rows of a logits operand fall into 16 different bank groups
//   logits  f32 MFMA 16x16x4 with B = (float)W[c][k] + a[c][k] formed in registers (W fp64 from L2 every step).  The
//           A operand of the Gram x_s.x_t of the minibatch rows is that same register as A and B: the Gram rides in
//           the same K-tile pass, one more MFMA per k step and no more LDS reads
//   clip    for a linear scorer ||g||^2 = sum_{s,t} (G_s.G_t)(x_s.x_t + 1) (dW = G^T x, db = sum_s G_s), so c_e is
//           known before dW exists: one (s, t) term per thread, combined in fp64 in a fixed order
//   dW      the MFMA pass (M = classes, N = k tile, K = samples) adds -lr c_e dW straight into a: every entry of a
//           is owned by one lane, there is no raw-gradient scratch and no second scaling pass
//   write   one pass at the end: delta (when a lived in LDS) and qdelta
// LDS: 17664 B tile + 8 KiB of per-wave partials + 4 KiB of draws + 1 KiB G = 31016 B static, plus at most 32 KiB
// of a (dynamic) = 62.3 KiB: inside the default 64 KiB, so no attribute is set at launch (a wider tile would save
// barriers, but mnist's a would no longer fit beside it without the opt-in).
// No atomics, no reduction whose order depends on timing: two runs give the same bytes.
// =====================================================================================
constexpr int LS_KT = 256;
constexpr int LS_KS = LS_KT + 20;
constexpr int LS_LDS_A = 8192;
constexpr int LS_MAX_E = 64;
// scalar fp32 code only in the new kernels (no packed fp32 instructions)
#define BSC_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))

namespace {
template <class Loss, bool A_IN_LDS>
BSC_NO_PK_F32 __global__ void __launch_bounds__(SM_THREADS) k_local_steps(
    const float* X, const int* y, const long long* off, const int* ntrain, const int* pid, const double* W, int D_IN,
    int D_OUT, int B, int P, unsigned long long seed, int iteration, float max_norm, double qscale, int E, float lr,
    float* delta, long long* qdelta, float* loss, int lo, int* ones, int nones) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  if (ones != nullptr && blockIdx.x == 0)
    for (int i = threadIdx.x; i < nones; i += blockDim.x) ones[i] = 1;
  extern __shared__ float ls_a[];         // [nparam] when A_IN_LDS, else unused (0 bytes)
  __shared__ float xs[16 * LS_KS];        // one K tile of the minibatch rows, transformed; rows >= Bq are zero
  __shared__ float red[4][16][16];        // per-wave partial logits [s][c]
  __shared__ float gram[4][16][16];       // per-wave partial Gram [s][t] of the transformed rows
  __shared__ float G[16][16];             // d(mean loss) / d(logits)
  __shared__ int bidx[LS_MAX_E][16];      // every step's minibatch
  __shared__ double nrm[SM_THREADS / 64];
  __shared__ float scale_sh;
  const int p = blockIdx.x;
  if (p >= P) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nparam = D_OUT * D_IN + D_OUT;
  const int li = lo >= 0 ? pid[p] - lo : p;
  const long long offp = off[li];
  const int n = ntrain[li];
  const int Bq = min(B, n);
  float* dst = delta + (size_t)p * nparam;
  float* a = A_IN_LDS ? ls_a : dst;
  // 1. the E minibatches (K1's draw under step e's tag), one lane per step; a_0 = 0
  if (tid < E) {
    int cnt = 0;
    uint32_t ctr = 0;
    const uint32_t tag = 0x5EEDu ^ ((uint32_t)tid << 16);
    while (cnt < Bq) {
      u4 r = philox(u4{(uint32_t)pid[p], (uint32_t)iteration, ctr++, tag}, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (cnt >= Bq) break;
        const int c = (int)((q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w) % (uint32_t)n);
        bool dup = false;
        for (int t = 0; t < cnt; ++t) dup |= bidx[tid][t] == c;
        if (!dup) bidx[tid][cnt++] = c;
      }
    }
    for (int t = cnt; t < 16; ++t) bidx[tid][t] = -1;
  }
  for (int i = tid; i < nparam; i += SM_THREADS) a[i] = 0.f;
  __syncthreads();
  const int ktiles = (D_IN + LS_KT - 1) / LS_KT;
  const int row = lane & 15, kk = lane >> 4;   // MFMA operand coordinates of this lane
  for (int e = 0; e < E; ++e) {
    const int* bi = bidx[e];
    auto stage = [&](int kt) __attribute__((always_inline)) {  // (x - 0.5) / 0.5; zero padding
      const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
      for (int i = tid; i < 16 * kw; i += SM_THREADS) {
        const int s = i / kw, k = i % kw;
        float v = 0.f;
        if (s < Bq) v = (X[(offp + bi[s]) * (long long)D_IN + k0 + k] - 0.5f) * 2.0f;
        xs[s * LS_KS + k] = v;
      }
    };
    // 2. logits of w_e = (float)W + a and the rows' Gram, in one pass over the K tiles (the 4 waves split a tile)
    {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f}, gacc = {0.f, 0.f, 0.f, 0.f};
      for (int kt = 0; kt < ktiles; ++kt) {
        const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
        __syncthreads();  // the tile's last readers (the previous tile, or the previous step's dW pass) are done
        stage(kt);
        __syncthreads();
        const int ksteps = (kw + 3) / 4;
        const int per = (ksteps + 3) / 4;
        for (int st = wid * per; st < min(ksteps, (wid + 1) * per); ++st) {
          const int k = st * 4 + kk;
          const bool in = k < kw;
          const float av = in ? xs[row * LS_KS + k] : 0.f;
          float bv = 0.f;
          if (in && row < D_OUT) bv = (float)W[row * D_IN + k0 + k] + a[row * D_IN + k0 + k];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
          gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, av, gacc, 0, 0, 0);   // A[s][k] and B[k][t]: one register
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[wid][kk * 4 + r][row] = acc[r];
        gram[wid][kk * 4 + r][row] = gacc[r];
      }
    }
    __syncthreads();
    // 3. the loss and G on rows s < Bq (one thread per row), as K1
    if (tid < 16) {
      const int s = tid;
      if (s < Bq) {
        float* lg = red[0][s];   // the row's logits, summed in place (LDS: the label indexes them)
        for (int c = 0; c < D_OUT; ++c)
          lg[c] = red[0][s][c] + red[1][s][c] + red[2][s][c] + red[3][s][c] +
                  ((float)W[D_OUT * D_IN + c] + a[D_OUT * D_IN + c]);
        const float l = Loss::row(lg, D_OUT, y[offp + bi[s]], Bq, G[s]);
        for (int c = D_OUT; c < 16; ++c) G[s][c] = 0.f;
        red[1][s][0] = l;
      } else {
        for (int c = 0; c < 16; ++c) G[s][c] = 0.f;
      }
    }
    __syncthreads();
    if (tid == 0 && e == E - 1) {
      float l = 0.f;
      for (int s = 0; s < Bq; ++s) l += red[1][s][0];
      loss[p] = l / (float)max(Bq, 1);
    }
    // 4. the clip coefficient from G and the Gram: thread (s, t) holds (G_s.G_t)(x_s.x_t + 1)
    {
      const int s = tid >> 4, t = tid & 15;
      double gg = 0.0;
#pragma unroll
      for (int c = 0; c < 16; ++c) gg += (double)G[s][c] * (double)G[t][c];
      const float xx = gram[0][s][t] + gram[1][s][t] + gram[2][s][t] + gram[3][s][t];
      double sq = gg * ((double)xx + 1.0);
      for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
      if (lane == 0) nrm[wid] = sq;
    }
    __syncthreads();
    if (tid == 0) {
      const float tot = (float)sqrt(fmax(nrm[0] + nrm[1] + nrm[2] + nrm[3], 0.0));
      const float coef = max_norm / (tot + 1e-6f);
      scale_sh = coef < 1.f ? coef : 1.f;
    }
    __syncthreads();
    const float sc = -(lr * scale_sh);
    // 5. a += sc * dW, dW[c][k] = sum_s G[s][c] xs[s][k] via f32 MFMA; the last tile is still resident: it goes first
    for (int q = 0; q < ktiles; ++q) {
      const int kt = (ktiles - 1 + q) % ktiles;
      const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
      if (q > 0) {
        __syncthreads();
        stage(kt);
        __syncthreads();
      }
      const int ntiles = (kw + 15) / 16;
      for (int t = wid; t < ntiles; t += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int k = t * 16 + row;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int s = ks * 4 + kk;
          const float av = G[s][row];  // A[c = row][s]
          const float bv = (k < kw) ? xs[s * LS_KS + k] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = kk * 4 + r;
          if (c < D_OUT && k < kw) a[c * D_IN + k0 + k] += sc * acc[r];
        }
      }
    }
    if (tid < D_OUT) {
      float db = 0.f;
      for (int s = 0; s < 16; ++s) db += G[s][tid];
      a[D_OUT * D_IN + tid] += sc * db;
    }
    // (the next step's first barrier, or the one below, orders these writes of a before their readers)
  }
  __syncthreads();
  // 6. delta = a_E, quantised like updateFloatToInt
  long long* qd = qdelta + (size_t)p * nparam;
  for (int i = tid; i < nparam; i += SM_THREADS) {
    const float v = a[i];
    if (A_IN_LDS) dst[i] = v;
    qd[i] = quantize(v, qscale);
  }
}
}  // namespace

// =====================================================================================
// K1m: K1e's E local steps under the reference clients' optimiser (--local-momentum M, --local-decay LAMBDA,
// --local-prox MU; docs/QUIRKS.md Q20): heavy-ball momentum m, weight decay lambda and a FedProx proximal weight mu.
//   a_0 = 0, v_0 = 0;  step e: w_e = (float)W + a_e, minibatch e (K1e's tags), g_e and c_e as K1e,
//   h_e = c_e g_e + lambda w_e + mu a_e (only the data gradient is clipped; the bias entries decay too),
//   v_{e+1} = m v_e + h_e (PyTorch's SGD: dampening 0, no Nesterov), a_{e+1} = a_e - lr v_{e+1};
//   delta = a_E (not clipped again), qdelta = quantize(delta), loss = the last step's mean row loss.
// K1e's workgroup, draws, 256-feature tile with its 20-float skew, logits + Gram pass and fp64 clip coefficient; what
// is its own:
//   v       MOM only: the velocity is a second resident vector beside a.  A_IN_LDS: in dynamic LDS behind a
//           (v = ls_a + nparam); else in the peer's row of the caller's fp32 [P, nparam] workspace vwork, which like
//           its delta row no other workgroup touches and which stays L2-hot.  v_0 = 0 is never stored: step 0 takes
//           its v as zero (a uniform branch), so the workspace needs no clearing and launches may share it
//   MOM=0   m = 0: there is no v at all, h_e goes straight into a; LDS and cost are K1e's, no workspace
//   update  fused into the dW MFMA pass: the lane that owns a[c][k] reads v[c][k], forms h from its accumulator, its
//           own a (and, when lambda != 0 -- a uniform branch -- (float)W[c][k] from L2 again), writes v and a.  Every
//           entry of a and v has one owner and every entry is met once per step (the tiles cover [D_OUT][D_IN]), so
//           the decay and proximal terms need no pass of their own, no raw-gradient scratch and no barrier; the
//           tid < D_OUT threads treat the bias entries the same way
// LDS: K1e's 31016 B static.  MOM = false: plus at most 32 KiB of a = 62.3 KiB, inside the default 64 KiB.  MOM = true
// and A_IN_LDS: plus at most 64 KiB of a and v = 94.3 KiB, raised once per instance with hipFuncSetAttribute (one
// workgroup per CU serves the 100 peers of a round: occupancy is not what bounds it).
// No atomics, no reduction whose order depends on timing: two runs give the same bytes.
// =====================================================================================
namespace {
template <class Loss, bool A_IN_LDS, bool MOM>
BSC_NO_PK_F32 __global__ void __launch_bounds__(SM_THREADS) k_momentum_steps(
    const float* X, const int* y, const long long* off, const int* ntrain, const int* pid, const double* W, int D_IN,
    int D_OUT, int B, int P, unsigned long long seed, int iteration, float max_norm, double qscale, int E, float lr,
    float mom, float decay, float prox, float* delta, long long* qdelta, float* loss, float* vwork, int lo, int* ones,
    int nones) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  if (ones != nullptr && blockIdx.x == 0)
    for (int i = threadIdx.x; i < nones; i += blockDim.x) ones[i] = 1;
  extern __shared__ float ls_a[];         // A_IN_LDS: a [nparam], then v [nparam] when MOM; else unused (0 bytes)
  __shared__ float xs[16 * LS_KS];        // one K tile of the minibatch rows, transformed; rows >= Bq are zero
  __shared__ float red[4][16][16];        // per-wave partial logits [s][c]
  __shared__ float gram[4][16][16];       // per-wave partial Gram [s][t] of the transformed rows
  __shared__ float G[16][16];             // d(mean loss) / d(logits)
  __shared__ int bidx[LS_MAX_E][16];      // every step's minibatch
  __shared__ double nrm[SM_THREADS / 64];
  __shared__ float scale_sh;
  const int p = blockIdx.x;
  if (p >= P) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nparam = D_OUT * D_IN + D_OUT;
  const int li = lo >= 0 ? pid[p] - lo : p;
  const long long offp = off[li];
  const int n = ntrain[li];
  const int Bq = min(B, n);
  float* dst = delta + (size_t)p * nparam;
  float* a = A_IN_LDS ? ls_a : dst;
  float* v = !MOM ? nullptr : A_IN_LDS ? ls_a + nparam : vwork + (size_t)p * nparam;
  const bool wd = decay != 0.f;
  // 1. the E minibatches, one lane per step, as K1e; a_0 = 0
  if (tid < E) {
    int cnt = 0;
    uint32_t ctr = 0;
    const uint32_t tag = 0x5EEDu ^ ((uint32_t)tid << 16);
    while (cnt < Bq) {
      u4 r = philox(u4{(uint32_t)pid[p], (uint32_t)iteration, ctr++, tag}, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (cnt >= Bq) break;
        const int c = (int)((q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w) % (uint32_t)n);
        bool dup = false;
        for (int t = 0; t < cnt; ++t) dup |= bidx[tid][t] == c;
        if (!dup) bidx[tid][cnt++] = c;
      }
    }
    for (int t = cnt; t < 16; ++t) bidx[tid][t] = -1;
  }
  for (int i = tid; i < nparam; i += SM_THREADS) a[i] = 0.f;
  __syncthreads();
  const int ktiles = (D_IN + LS_KT - 1) / LS_KT;
  const int row = lane & 15, kk = lane >> 4;   // MFMA operand coordinates of this lane
  for (int e = 0; e < E; ++e) {
    const int* bi = bidx[e];
    auto stage = [&](int kt) __attribute__((always_inline)) {  // (x - 0.5) / 0.5; zero padding
      const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
      for (int i = tid; i < 16 * kw; i += SM_THREADS) {
        const int s = i / kw, k = i % kw;
        float xv = 0.f;
        if (s < Bq) xv = (X[(offp + bi[s]) * (long long)D_IN + k0 + k] - 0.5f) * 2.0f;
        xs[s * LS_KS + k] = xv;
      }
    };
    // the owner's update of entry i from its clipped data gradient cg = c_e g_e[i]: h, then v (MOM) and a
    auto update = [&](int i, float cg) __attribute__((always_inline)) {
      const float ai = a[i];
      float h = cg + prox * ai;
      if (wd) h += decay * ((float)W[i] + ai);
      if (MOM) {
        if (e > 0) h += mom * v[i];
        v[i] = h;
      }
      a[i] = ai - lr * h;
    };
    // 2. logits of w_e = (float)W + a and the rows' Gram, in one pass over the K tiles (the 4 waves split a tile)
    {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f}, gacc = {0.f, 0.f, 0.f, 0.f};
      for (int kt = 0; kt < ktiles; ++kt) {
        const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
        __syncthreads();  // the tile's last readers (the previous tile, or the previous step's dW pass) are done
        stage(kt);
        __syncthreads();
        const int ksteps = (kw + 3) / 4;
        const int per = (ksteps + 3) / 4;
        for (int st = wid * per; st < min(ksteps, (wid + 1) * per); ++st) {
          const int k = st * 4 + kk;
          const bool in = k < kw;
          const float av = in ? xs[row * LS_KS + k] : 0.f;
          float bv = 0.f;
          if (in && row < D_OUT) bv = (float)W[row * D_IN + k0 + k] + a[row * D_IN + k0 + k];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
          gacc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, av, gacc, 0, 0, 0);   // A[s][k] and B[k][t]: one register
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        red[wid][kk * 4 + r][row] = acc[r];
        gram[wid][kk * 4 + r][row] = gacc[r];
      }
    }
    __syncthreads();
    // 3. the loss and G on rows s < Bq (one thread per row), as K1
    if (tid < 16) {
      const int s = tid;
      if (s < Bq) {
        float* lg = red[0][s];   // the row's logits, summed in place (LDS: the label indexes them)
        for (int c = 0; c < D_OUT; ++c)
          lg[c] = red[0][s][c] + red[1][s][c] + red[2][s][c] + red[3][s][c] +
                  ((float)W[D_OUT * D_IN + c] + a[D_OUT * D_IN + c]);
        const float l = Loss::row(lg, D_OUT, y[offp + bi[s]], Bq, G[s]);
        for (int c = D_OUT; c < 16; ++c) G[s][c] = 0.f;
        red[1][s][0] = l;
      } else {
        for (int c = 0; c < 16; ++c) G[s][c] = 0.f;
      }
    }
    __syncthreads();
    if (tid == 0 && e == E - 1) {
      float l = 0.f;
      for (int s = 0; s < Bq; ++s) l += red[1][s][0];
      loss[p] = l / (float)max(Bq, 1);
    }
    // 4. the clip coefficient from G and the Gram: thread (s, t) holds (G_s.G_t)(x_s.x_t + 1)
    {
      const int s = tid >> 4, t = tid & 15;
      double gg = 0.0;
#pragma unroll
      for (int c = 0; c < 16; ++c) gg += (double)G[s][c] * (double)G[t][c];
      const float xx = gram[0][s][t] + gram[1][s][t] + gram[2][s][t] + gram[3][s][t];
      double sq = gg * ((double)xx + 1.0);
      for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
      if (lane == 0) nrm[wid] = sq;
    }
    __syncthreads();
    if (tid == 0) {
      const float tot = (float)sqrt(fmax(nrm[0] + nrm[1] + nrm[2] + nrm[3], 0.0));
      const float coef = max_norm / (tot + 1e-6f);
      scale_sh = coef < 1.f ? coef : 1.f;
    }
    __syncthreads();
    const float sc = scale_sh;
    // 5. dW[c][k] = sum_s G[s][c] xs[s][k] via f32 MFMA, each entry's owner applying the update from its accumulator;
    // the last tile is still resident: it goes first
    for (int q = 0; q < ktiles; ++q) {
      const int kt = (ktiles - 1 + q) % ktiles;
      const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
      if (q > 0) {
        __syncthreads();
        stage(kt);
        __syncthreads();
      }
      const int ntiles = (kw + 15) / 16;
      for (int t = wid; t < ntiles; t += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int k = t * 16 + row;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int s = ks * 4 + kk;
          const float av = G[s][row];  // A[c = row][s]
          const float bv = (k < kw) ? xs[s * LS_KS + k] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = kk * 4 + r;
          if (c < D_OUT && k < kw) update(c * D_IN + k0 + k, sc * acc[r]);
        }
      }
    }
    if (tid < D_OUT) {
      float db = 0.f;
      for (int s = 0; s < 16; ++s) db += G[s][tid];
      update(D_OUT * D_IN + tid, sc * db);
    }
    // (the next step's first barrier, or the one below, orders these writes of a before their readers; v has no
    // reader but its owner)
  }
  __syncthreads();
  // 6. delta = a_E, quantised like updateFloatToInt
  long long* qd = qdelta + (size_t)p * nparam;
  for (int i = tid; i < nparam; i += SM_THREADS) {
    const float r = a[i];
    if (A_IN_LDS) dst[i] = r;
    qd[i] = quantize(r, qscale);
  }
}
}  // namespace

// =====================================================================================
// K1p: E DP-SGD steps of the same linear scorer per round (--dp-clip C [--dp-sigma S]; docs/QUIRKS.md Q18): each
// example's gradient is clipped to C before the minibatch rows are summed, N(0, (S C)^2) is added to the sum, and
// the sum is divided by the batch size.
//   a_0 = 0;  step e: w_e = (float)W + a_e, minibatch e (K1e's tags), gamma_s = Bq G_s the row's gradient with
//   respect to its logits, n_s = ||gamma_s|| sqrt(||x_s||^2 + 1), c_s = min(1, C / (n_s + 1e-6)),
//   g_e = (1 / Bq) (sum_s c_s gamma_s (x) (x_s, 1) + S C xi_e), a_{e+1} = a_e - lr g_e (no clip of the mean);
//   xi_e[j] = gauss of philox((j, iteration, peer, 0xD95D ^ (e << 16)), seed);  delta = a_E, qdelta, the last loss.
// K1e's workgroup, residency of a, draws and 256-feature tile; what is its own:
//   norms   a row's gradient has rank one, so n_s needs ||x_s||^2 and nothing of dW: every lane squares the A operand
//           it already holds beside the logits MFMA (one FMA per k step in place of K1e's Gram MFMA), the four kk lane
//           groups meet through two __shfl_xor, the four waves through rsq[4][16], summed in a fixed order
//   clip    the row thread that runs Loss::row scales its row of G by c_s in place: the dW pass then sums clipped
//           rows at K1e's cost, and there is no norm of the whole gradient, no fp64 and no second barrier pair
//   noise   S > 0 only (a uniform branch): one pass over a per step, one Philox call per entry; the last step's
//           pass is the final delta / qdelta write
// LDS: 17664 B tile + 4 KiB of per-wave logits + 256 B of row norms + 4 KiB of draws + 1 KiB G = 27136 B static,
// plus at most 32 KiB of a (dynamic) = 58.5 KiB: inside the default 64 KiB, no attribute is set at launch.
// No atomics, no reduction whose order depends on timing: two runs give the same bytes.
// =====================================================================================
namespace {
template <class Loss, bool A_IN_LDS>
BSC_NO_PK_F32 __global__ void __launch_bounds__(SM_THREADS) k_dpsgd_steps(
    const float* X, const int* y, const long long* off, const int* ntrain, const int* pid, const double* W, int D_IN,
    int D_OUT, int B, int P, unsigned long long seed, int iteration, double qscale, float clip, float sigma, int E,
    float lr, float* delta, long long* qdelta, float* loss, int lo, int* ones, int nones) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  if (ones != nullptr && blockIdx.x == 0)
    for (int i = threadIdx.x; i < nones; i += blockDim.x) ones[i] = 1;
  extern __shared__ float dp_a[];         // [nparam] when A_IN_LDS, else unused (0 bytes)
  __shared__ float xs[16 * LS_KS];        // one K tile of the minibatch rows, transformed; rows >= Bq are zero
  __shared__ float red[4][16][16];        // per-wave partial logits [s][c]
  __shared__ float rsq[4][16];            // per-wave partial ||x_s||^2
  __shared__ float G[16][16];             // c_s G_s: the clipped rows of d(mean loss) / d(logits)
  __shared__ int bidx[LS_MAX_E][16];      // every step's minibatch
  const int p = blockIdx.x;
  if (p >= P) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nparam = D_OUT * D_IN + D_OUT;
  const uint32_t peer = (uint32_t)pid[p];
  const int li = lo >= 0 ? pid[p] - lo : p;
  const long long offp = off[li];
  const int n = ntrain[li];
  const int Bq = min(B, n);
  float* dst = delta + (size_t)p * nparam;
  float* a = A_IN_LDS ? dp_a : dst;
  const uint32_t k0s = (uint32_t)seed, k1s = (uint32_t)(seed >> 32);
  // 1. the E minibatches, one lane per step (K1e's draw); a_0 = 0
  if (tid < E) {
    int cnt = 0;
    uint32_t ctr = 0;
    const uint32_t tag = 0x5EEDu ^ ((uint32_t)tid << 16);
    while (cnt < Bq) {
      u4 r = philox(u4{peer, (uint32_t)iteration, ctr++, tag}, k0s, k1s);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (cnt >= Bq) break;
        const int c = (int)((q == 0 ? r.x : q == 1 ? r.y : q == 2 ? r.z : r.w) % (uint32_t)n);
        bool dup = false;
        for (int t = 0; t < cnt; ++t) dup |= bidx[tid][t] == c;
        if (!dup) bidx[tid][cnt++] = c;
      }
    }
    for (int t = cnt; t < 16; ++t) bidx[tid][t] = -1;
  }
  for (int i = tid; i < nparam; i += SM_THREADS) a[i] = 0.f;
  __syncthreads();
  const int ktiles = (D_IN + LS_KT - 1) / LS_KT;
  const int row = lane & 15, kk = lane >> 4;   // MFMA operand coordinates of this lane
  const bool noisy = sigma > 0.f;              // uniform
  const float nsc = lr * (sigma * clip / (float)max(Bq, 1));   // what one N(0, 1) draw moves an entry of a by
  auto xi = [&](int j, int e) __attribute__((always_inline)) {
    const u4 r = philox(u4{(uint32_t)j, (uint32_t)iteration, peer, 0xD95Du ^ ((uint32_t)e << 16)}, k0s, k1s);
    return gauss(r.x, r.y);
  };
  for (int e = 0; e < E; ++e) {
    const int* bi = bidx[e];
    auto stage = [&](int kt) __attribute__((always_inline)) {  // (x - 0.5) / 0.5; zero padding
      const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
      for (int i = tid; i < 16 * kw; i += SM_THREADS) {
        const int s = i / kw, k = i % kw;
        float v = 0.f;
        if (s < Bq) v = (X[(offp + bi[s]) * (long long)D_IN + k0 + k] - 0.5f) * 2.0f;
        xs[s * LS_KS + k] = v;
      }
    };
    // 2. logits of w_e = (float)W + a and the rows' squared norms, in one pass over the K tiles
    {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      float xx = 0.f;   // this lane's share of ||x_row||^2: the k of its kk group in its wave's part of each tile
      for (int kt = 0; kt < ktiles; ++kt) {
        const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
        __syncthreads();  // the tile's last readers and the last writers of a (dW or noise pass) are done
        stage(kt);
        __syncthreads();
        const int ksteps = (kw + 3) / 4;
        const int per = (ksteps + 3) / 4;
        for (int st = wid * per; st < min(ksteps, (wid + 1) * per); ++st) {
          const int k = st * 4 + kk;
          const bool in = k < kw;
          const float av = in ? xs[row * LS_KS + k] : 0.f;
          float bv = 0.f;
          if (in && row < D_OUT) bv = (float)W[row * D_IN + k0 + k] + a[row * D_IN + k0 + k];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
          xx = fmaf(av, av, xx);
        }
      }
      xx += __shfl_xor(xx, 16);
      xx += __shfl_xor(xx, 32);
      if (kk == 0) rsq[wid][row] = xx;
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wid][kk * 4 + r][row] = acc[r];
    }
    __syncthreads();
    // 3. the loss, G and the clip on rows s < Bq (one thread per row): the row of G leaves scaled by c_s
    if (tid < 16) {
      const int s = tid;
      if (s < Bq) {
        float* lg = red[0][s];   // the row's logits, summed in place (LDS: the label indexes them)
        for (int c = 0; c < D_OUT; ++c)
          lg[c] = red[0][s][c] + red[1][s][c] + red[2][s][c] + red[3][s][c] +
                  ((float)W[D_OUT * D_IN + c] + a[D_OUT * D_IN + c]);
        const float l = Loss::row(lg, D_OUT, y[offp + bi[s]], Bq, G[s]);
        float gg = 0.f;
        for (int c = 0; c < D_OUT; ++c) gg = fmaf(G[s][c], G[s][c], gg);
        const float x2 = (rsq[0][s] + rsq[1][s]) + (rsq[2][s] + rsq[3][s]);
        const float ns = (float)Bq * sqrtf(gg) * sqrtf(x2 + 1.f);   // ||gamma_s (x) (x_s, 1)||, gamma_s = Bq G_s
        const float coef = clip / (ns + 1e-6f);
        if (coef < 1.f)
          for (int c = 0; c < D_OUT; ++c) G[s][c] *= coef;
        for (int c = D_OUT; c < 16; ++c) G[s][c] = 0.f;
        red[1][s][0] = l;
      } else {
        for (int c = 0; c < 16; ++c) G[s][c] = 0.f;
      }
    }
    __syncthreads();
    if (tid == 0 && e == E - 1) {
      float l = 0.f;
      for (int s = 0; s < Bq; ++s) l += red[1][s][0];
      loss[p] = l / (float)max(Bq, 1);
    }
    const float sc = -lr;
    // 4. a += sc * dW, dW[c][k] = sum_s G[s][c] xs[s][k] (clipped rows) via f32 MFMA; the resident last tile goes first
    for (int q = 0; q < ktiles; ++q) {
      const int kt = (ktiles - 1 + q) % ktiles;
      const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
      if (q > 0) {
        __syncthreads();
        stage(kt);
        __syncthreads();
      }
      const int ntiles = (kw + 15) / 16;
      for (int t = wid; t < ntiles; t += 4) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int k = t * 16 + row;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const int s = ks * 4 + kk;
          const float av = G[s][row];  // A[c = row][s]
          const float bv = (k < kw) ? xs[s * LS_KS + k] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = kk * 4 + r;
          if (c < D_OUT && k < kw) a[c * D_IN + k0 + k] += sc * acc[r];
        }
      }
    }
    if (tid < D_OUT) {
      float db = 0.f;
      for (int s = 0; s < 16; ++s) db += G[s][tid];
      a[D_OUT * D_IN + tid] += sc * db;
    }
    // 5. the step's noise, a -= lr (S C / Bq) xi_e; the last step's goes into the write below
    if (noisy && e < E - 1) {
      __syncthreads();   // the dW pass owns entries of a by lane, this pass by index
      for (int i = tid; i < nparam; i += SM_THREADS) a[i] -= nsc * xi(i, e);
    }
    // (the next step's first barrier, or the one below, orders these writes of a before their readers)
  }
  __syncthreads();
  // 6. delta = a_E (with the last step's noise), quantised like updateFloatToInt
  long long* qd = qdelta + (size_t)p * nparam;
  for (int i = tid; i < nparam; i += SM_THREADS) {
    float v = a[i];
    if (noisy) v -= nsc * xi(i, E - 1);
    if (A_IN_LDS || noisy) dst[i] = v;
    qd[i] = quantize(v, qscale);
  }
}
}  // namespace

// =====================================================================================
// K1l: E local steps on lots of up to LOT_MAX = 256 examples (--lot-size L; docs/QUIRKS.md Q19).  K1e's rule
// (DP = false: clip of the mean at max_norm) or K1p's (DP = true: per-example clip, noise on the clipped sum) with
// Lq = min(L, n) rows per step in place of Bq <= 16; draws, tags, scorer, noise counters and outputs are theirs.
// One 256-thread workgroup per peer; the lot, not a 16-row MFMA tile, is the unit of a step:
//   draw    per step (E * L indices do not fit), by wave 0.  The 64 lanes run Philox for 64 counters at once and
//           reduce their 256 candidates mod n; the candidates are then taken in the reference's order, each broadcast
//           and tested against the accepted indices -- held four per lane over the wave -- by four compares and one
//           ballot, so the rejection rule yields minibatch_indices' exact sequence.  n <= L: the shard is taken whole
//           in storage order (the draw's order only decides which rows share a tile; the sums do not depend on it)
//   pass A  row tile by row tile: K1p's logits pass (LS_KT-wide tiles, f32 MFMA 16x16x4, B = (float)W + a formed in
//           registers; under DP ||x_s||^2 by one FMA per k step), then Loss::row by one thread per row.  The lot's
//           whole G [256][16] stays in LDS, under DP with c_s already folded into its rows
//   pass B  K tile by K tile, the lot as the MFMA's K dimension: every row tile of the K tile is staged again (the
//           rows are L2-hot) while a wave's four 16-column accumulators stay in registers, so dW[c][k] has MFMA depth
//           Lq and is finished once, by the one lane that owns it.  DP: the finished entry takes its noise and -lr
//           and goes straight into a (pass A is over: in place is safe; there is no gradient buffer).  Else it goes
//           into the step gradient g and its square into the lane's share of ||g||^2 (fp64; lanes, then waves, in a
//           fixed order); once the norm is known a last pass does a -= lr c g
//   a, g    in LDS when nparam <= LS_LDS_A (g behind a), else a is the peer's delta row and g its row of the
//           launcher's [P, nparam] workspace
// LDS: 17664 B tile + 4 KiB of per-wave logits + 16 KiB G + 1 KiB of indices + 64 B of losses + 256 B of row norms
// (DP) or 32 B of norm partials (not DP) = 39488 / 39264 B static, plus a (DP: at most 32 KiB) or a and g (at most
// 64 KiB) dynamic: up to 70.6 KiB under DP and 102.3 KiB without, above the default 64 KiB and inside gfx950's
// 160 KiB per workgroup (one workgroup per CU; a round launches one per peer).  The launcher raises the dynamic
// limit of the two A_IN_LDS instances once, with hipFuncSetAttribute, and returns its error if that fails.
// No atomics, no reduction whose order depends on timing: two runs give the same bytes.
// =====================================================================================
constexpr int LOT_MAX = 256;

namespace {
template <class Loss, bool A_IN_LDS, bool DP>
BSC_NO_PK_F32 __global__ void __launch_bounds__(SM_THREADS) k_lot_steps(
    const float* X, const int* y, const long long* off, const int* ntrain, const int* pid, const double* W, int D_IN,
    int D_OUT, int L, int P, unsigned long long seed, int iteration, float max_norm, double qscale, float clip,
    float sigma, int E, float lr, float* delta, long long* qdelta, float* loss, float* gwork, int lo, int* ones,
    int nones) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  if (ones != nullptr && blockIdx.x == 0)
    for (int i = threadIdx.x; i < nones; i += blockDim.x) ones[i] = 1;
  extern __shared__ float lot_ag[];       // A_IN_LDS: a [nparam], then (not DP) g [nparam]; else unused (0 bytes)
  __shared__ float xs[16 * LS_KS];        // one K tile of one row tile, transformed; rows >= Lq are zero
  __shared__ float red[4][16][16];        // per-wave partial logits [s][c] of the row tile
  __shared__ float rsq[4][16];            // per-wave partial ||x_s||^2 (DP)
  __shared__ float G[LOT_MAX][16];        // the lot's (c_s) d(mean loss) / d(logits); rows >= Lq of the last tile: 0
  __shared__ int idx[LOT_MAX];            // this step's lot
  __shared__ float rl[16];                // the row threads' loss sums
  __shared__ double nrm[SM_THREADS / 64];
  const int p = blockIdx.x;
  if (p >= P) return;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int nw = D_OUT * D_IN, nparam = nw + D_OUT;
  const uint32_t peer = (uint32_t)pid[p];
  const int li = lo >= 0 ? pid[p] - lo : p;
  const long long offp = off[li];
  const int n = ntrain[li];
  const int Lq = min(L, n);
  const int rtiles = (Lq + 15) / 16;
  float* dst = delta + (size_t)p * nparam;
  float* a = A_IN_LDS ? lot_ag : dst;
  float* g = DP ? nullptr : A_IN_LDS ? lot_ag + nparam : gwork + (size_t)p * nparam;
  const uint32_t k0s = (uint32_t)seed, k1s = (uint32_t)(seed >> 32);
  for (int i = tid; i < nparam; i += SM_THREADS) a[i] = 0.f;
  const int ktiles = (D_IN + LS_KT - 1) / LS_KT;
  const int row = lane & 15, kk = lane >> 4;   // MFMA operand coordinates of this lane
  const bool noisy = DP && sigma > 0.f;        // uniform
  const float nsc = lr * (sigma * clip / (float)max(Lq, 1));   // what one N(0, 1) draw moves an entry of a by
  auto xi = [&](int j, int e) __attribute__((always_inline)) {
    const u4 r = philox(u4{(uint32_t)j, (uint32_t)iteration, peer, 0xD95Du ^ ((uint32_t)e << 16)}, k0s, k1s);
    return gauss(r.x, r.y);
  };
  auto stage = [&](int rt, int kt) __attribute__((always_inline)) {  // (x - 0.5) / 0.5; zero padding
    const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
    for (int i = tid; i < 16 * kw; i += SM_THREADS) {
      const int sl = i / kw, k = i % kw, s = rt * 16 + sl;
      float v = 0.f;
      if (s < Lq) v = (X[(offp + idx[s]) * (long long)D_IN + k0 + k] - 0.5f) * 2.0f;
      xs[sl * LS_KS + k] = v;
    }
  };
  for (int e = 0; e < E; ++e) {
    __syncthreads();   // the last step's readers of idx and writers of a are done
    // 1. the step's lot: minibatch_indices(peer, iteration, n, L, seed, tag) by wave 0
    if (wid == 0) {
      if (n <= L) {
        for (int i = lane; i < Lq; i += 64) idx[i] = i;
      } else {
        const uint32_t tag = 0x5EEDu ^ ((uint32_t)e << 16);
        int h0 = -1, h1 = -1, h2 = -1, h3 = -1;   // accepted index j lives in lane j & 63, register j >> 6
        int cnt = 0;
        for (uint32_t ctr = 0; cnt < Lq; ctr += 64) {
          const u4 r = philox(u4{peer, (uint32_t)iteration, ctr + (uint32_t)lane, tag}, k0s, k1s);
          const int c0 = (int)(r.x % (uint32_t)n), c1 = (int)(r.y % (uint32_t)n), c2 = (int)(r.z % (uint32_t)n),
                    c3 = (int)(r.w % (uint32_t)n);
          for (int sl = 0; sl < 64 && cnt < Lq; ++sl) {
            const int q4[4] = {__shfl(c0, sl), __shfl(c1, sl), __shfl(c2, sl), __shfl(c3, sl)};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int c = q4[q];
              const bool dup = (h0 == c) | (h1 == c) | (h2 == c) | (h3 == c);
              if (cnt < Lq && __ballot(dup) == 0ull) {   // uniform: cnt and the ballot are the same in every lane
                if (lane == (cnt & 63)) {
                  const int w = cnt >> 6;
                  h0 = w == 0 ? c : h0;
                  h1 = w == 1 ? c : h1;
                  h2 = w == 2 ? c : h2;
                  h3 = w == 3 ? c : h3;
                  idx[cnt] = c;
                }
                ++cnt;
              }
            }
          }
        }
      }
    }
    __syncthreads();
    // 2. pass A: per row tile the logits of w_e = (float)W + a (and the rows' squared norms), then the loss and G
    float lsum = 0.f;
    for (int rt = 0; rt < rtiles; ++rt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      float xx = 0.f;   // this lane's share of ||x_row||^2
      for (int kt = 0; kt < ktiles; ++kt) {
        const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
        __syncthreads();  // the tile's last readers are done
        stage(rt, kt);
        __syncthreads();
        const int ksteps = (kw + 3) / 4;
        const int per = (ksteps + 3) / 4;
        for (int st = wid * per; st < min(ksteps, (wid + 1) * per); ++st) {
          const int k = st * 4 + kk;
          const bool in = k < kw;
          const float av = in ? xs[row * LS_KS + k] : 0.f;
          float bv = 0.f;
          if (in && row < D_OUT) bv = (float)W[row * D_IN + k0 + k] + a[row * D_IN + k0 + k];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
          if (DP) xx = fmaf(av, av, xx);
        }
      }
      if (DP) {
        xx += __shfl_xor(xx, 16);
        xx += __shfl_xor(xx, 32);
        if (kk == 0) rsq[wid][row] = xx;
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wid][kk * 4 + r][row] = acc[r];
      __syncthreads();
      // one thread per row of the tile; red and rsq are next written behind the next tile's staging barriers
      if (tid < 16) {
        const int s = rt * 16 + tid;
        if (s < Lq) {
          float* lg = red[0][tid];   // the row's logits, summed in place (LDS: the label indexes them)
          for (int c = 0; c < D_OUT; ++c)
            lg[c] = red[0][tid][c] + red[1][tid][c] + red[2][tid][c] + red[3][tid][c] +
                    ((float)W[nw + c] + a[nw + c]);
          lsum += Loss::row(lg, D_OUT, y[offp + idx[s]], Lq, G[s]);
          if (DP) {
            float gg = 0.f;
            for (int c = 0; c < D_OUT; ++c) gg = fmaf(G[s][c], G[s][c], gg);
            const float x2 = (rsq[0][tid] + rsq[1][tid]) + (rsq[2][tid] + rsq[3][tid]);
            const float ns = (float)Lq * sqrtf(gg) * sqrtf(x2 + 1.f);   // ||gamma_s (x) (x_s, 1)||, gamma_s = Lq G_s
            const float coef = clip / (ns + 1e-6f);
            if (coef < 1.f)
              for (int c = 0; c < D_OUT; ++c) G[s][c] *= coef;
          }
          for (int c = D_OUT; c < 16; ++c) G[s][c] = 0.f;
        } else {
          for (int c = 0; c < 16; ++c) G[s][c] = 0.f;
        }
      }
    }
    if (tid < 16) rl[tid] = lsum;
    __syncthreads();   // G is complete
    if (tid == 0 && e == E - 1) {
      float l = 0.f;
      for (int s = 0; s < 16; ++s) l += rl[s];
      loss[p] = l / (float)max(Lq, 1);
    }
    // 3. pass B: dW[c][k] = sum_{s < Lq} G[s][c] xs[s][k], K tile by K tile; wave w owns column tiles w, w + 4, ...
    double sq = 0.0;   // this lane's share of ||g||^2 (not DP)
    auto finish = [&](int i, float v) __attribute__((always_inline)) {
      if (DP) {
        float u = a[i] - lr * v;
        if (noisy) u -= nsc * xi(i, e);
        a[i] = u;
      } else {
        g[i] = v;
        sq += (double)v * (double)v;
      }
    };
    for (int kt = 0; kt < ktiles; ++kt) {
      const int k0 = kt * LS_KT, kw = min(LS_KT, D_IN - k0);
      const int ntiles = (kw + 15) / 16;
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int rt = 0; rt < rtiles; ++rt) {
        __syncthreads();
        stage(rt, kt);
        __syncthreads();
        float av[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) av[ks] = G[rt * 16 + ks * 4 + kk][row];   // A[c = row][s]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = (wid + 4 * j) * 16 + row;
          if (wid + 4 * j < ntiles) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
              const float bv = (k < kw) ? xs[(ks * 4 + kk) * LS_KS + k] : 0.f;
              acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ks], bv, acc[j], 0, 0, 0);
            }
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = (wid + 4 * j) * 16 + row;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = kk * 4 + r;
          if (c < D_OUT && k < kw) finish(c * D_IN + k0 + k, acc[j][r]);
        }
      }
    }
    if (tid < D_OUT) {
      float db = 0.f;
      for (int s = 0; s < rtiles * 16; ++s) db += G[s][tid];
      finish(nw + tid, db);
    }
    // 4. not DP: the clip of the mean from ||g||, then a -= lr c g
    if (!DP) {
      for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
      if (lane == 0) nrm[wid] = sq;
      __syncthreads();   // also: pass B owns entries of g by lane, this pass by index
      const float tot = (float)sqrt((nrm[0] + nrm[1]) + (nrm[2] + nrm[3]));
      const float coef = max_norm / (tot + 1e-6f);
      const float sc = -(lr * (coef < 1.f ? coef : 1.f));
      for (int i = tid; i < nparam; i += SM_THREADS) a[i] += sc * g[i];
    }
  }
  __syncthreads();
  // 5. delta = a_E, quantised like updateFloatToInt
  long long* qd = qdelta + (size_t)p * nparam;
  for (int i = tid; i < nparam; i += SM_THREADS) {
    const float v = a[i];
    if (A_IN_LDS) dst[i] = v;
    qd[i] = quantize(v, qscale);
  }
}
}  // namespace

// =====================================================================================
// K1t: top-k sparsification of the step's rows, in place (the reference's theta, ML/code/linear_model.py:48-88).
// Row p keeps its k entries of largest fp32 magnitude -- key(j) = bits(delta[j]) & 0x7fffffff, monotone as an
// integer; ties at the k-th key are kept in ascending index order -- and every other entry becomes delta = 0.0f,
// qdelta = 0.  An exact selection, not a sort: an MSB-first radix select over 8-bit digits.
//   load    the row's keys into LDS when they fit (KEYS_IN_LDS; else every pass re-reads the L2-hot row)
//   select  at most 4 passes.  Each wave counts the digit of the keys still matching the chosen prefix into its own
//           256-bin LDS histogram (integer atomics: the counts do not depend on order); wave 0 merges the four, one
//           lane per 4 bins, suffix-scans them with __shfl_down and picks the bin that holds the r-th largest
//           candidate; r becomes the number still to take from that bin.  A bin with exactly r keys ends the
//           passes: all of it is kept
//   write   in index order, 256 entries at a time: keep key > T; of the keys == T (T = the prefix, under the mask
//           of the digits chosen) the first r by index -- __ballot / __popcll ranks inside a wave, the waves'
//           counts through LDS, a running base across chunks, dropped once the r ties are placed.  The zeros are
//           plain stores, 512 contiguous bytes of qdelta per wave.  kept[p] (optional) = the row's non-zero qdelta
//           entries afterwards, one store per row.
// One 256-thread workgroup per row, no global atomics: two runs give the same bytes.
// =====================================================================================
constexpr int TK_THREADS = 256;
constexpr int TK_WAVES = TK_THREADS / 64;
constexpr int TK_LDS_KEYS = 14336;   // 56 KiB of keys beside the 4 KiB of histograms: inside the default 64 KiB

namespace {
template <bool KEYS_IN_LDS>
__device__ __forceinline__ void topk_row_body(float* delta, long long* qdelta, int D, int k, int* kept) {
  extern __shared__ uint32_t tk_keys[];             // [D] when KEYS_IN_LDS, else unused (0 bytes)
  __shared__ unsigned int hist[TK_WAVES][256];
  __shared__ unsigned int sel[3];                   // the chosen bin, the r left inside it, the bin's count
  __shared__ unsigned int wcnt[2][TK_WAVES];        // the final pass's ties per wave, double-buffered
  __shared__ int nz_w[TK_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* drow = delta + (size_t)blockIdx.x * D;
  long long* qrow = qdelta + (size_t)blockIdx.x * D;
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(drow);
  auto key_at = [&](int j) -> uint32_t { return KEYS_IN_LDS ? tk_keys[j] : (bits[j] & 0x7fffffffu); };

  if (KEYS_IN_LDS) {
    for (int j = tid; j < D; j += TK_THREADS) tk_keys[j] = bits[j] & 0x7fffffffu;
  }
  uint32_t prefix = 0, mask = 0;   // candidates: (key & mask) == prefix
  unsigned int r = (unsigned int)k;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < TK_WAVES * 256; i += TK_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();               // (also: the keys are in LDS before the first pass reads them)
    for (int j = tid; j < D; j += TK_THREADS) {
      const uint32_t key = key_at(j);
      if ((key & mask) == prefix) atomicAdd(&hist[wave][(key >> shift) & 0xffu], 1u);
    }
    __syncthreads();
    if (wave == 0) {
      unsigned int c[4], t = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        c[i] = 0;
#pragma unroll
        for (int w = 0; w < TK_WAVES; ++w) c[i] += hist[w][4 * lane + i];
        t += c[i];
      }
      unsigned int s = t;          // inclusive suffix sum over the lanes: candidates in bins >= 4 * lane
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned int v = __shfl_down(s, o);
        if (lane + o < 64) s += v;
      }
      unsigned int above = s - t;  // candidates in bins above this lane's four
#pragma unroll
      for (int i = 3; i >= 0; --i) {
        if (above < r && r <= above + c[i]) {   // true for exactly one bin of one lane (r <= the candidates)
          sel[0] = 4u * lane + i;
          sel[1] = r - above;
          sel[2] = c[i];
        }
        above += c[i];
      }
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    mask |= 0xffu << shift;
    r = sel[1];
    if (sel[2] == r) break;        // the whole bin is kept: no tie to break below this digit
  }

  // keep (key & mask) > prefix, and the first r of (key & mask) == prefix by index
  unsigned int base = 0;           // ties seen in the chunks before this one (the same in every thread)
  int nz = 0, buf = 0;
  for (int j0 = 0; j0 < D; j0 += TK_THREADS) {
    const int j = j0 + tid;
    const bool valid = j < D;
    const uint32_t km = valid ? (key_at(j) & mask) : 0u;
    bool keep = valid && km > prefix;
    if (base < r) {                // uniform: ties are still being placed
      const bool tie = valid && km == prefix;
      const unsigned long long b = __ballot(tie);
      if (lane == 0) wcnt[buf][wave] = (unsigned int)__popcll(b);
      __syncthreads();
      unsigned int before = base, all = 0;
#pragma unroll
      for (int w = 0; w < TK_WAVES; ++w) {
        const unsigned int n = wcnt[buf][w];
        if (w < wave) before += n;
        all += n;
      }
      keep |= tie && before + (unsigned int)__popcll(b & ((1ull << lane) - 1ull)) < r;
      base += all;
      buf ^= 1;                    // the next chunk's counts go to the other buffer: one barrier per chunk
    }
    if (valid) {
      if (!keep) {
        drow[j] = 0.0f;
        qrow[j] = 0;
      } else if (kept != nullptr) {
        nz += qrow[j] != 0;
      }
    }
  }
  if (kept != nullptr) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nz += __shfl_down(nz, o);
    if (lane == 0) nz_w[wave] = nz;
    __syncthreads();
    if (tid == 0) {
      int n = 0;
      for (int w = 0; w < TK_WAVES; ++w) n += nz_w[w];
      kept[blockIdx.x] = n;
    }
  }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(TK_THREADS) k_topk_rows(float* delta, long long* qdelta, int D, int k,
                                                                    int* kept) {
  topk_row_body<true>(delta, qdelta, D, k, kept);
}

// the same selection for a row too long for LDS (lfw: 17486 keys): every pass reads the keys from the row
extern "C" __global__ void __launch_bounds__(TK_THREADS) k_topk_rows_stream(float* delta, long long* qdelta, int D,
                                                                           int k, int* kept) {
  topk_row_body<false>(delta, qdelta, D, k, kept);
}

// =====================================================================================
// K3: logistic regression step (creditcard path).  One wave per peer.
// X: [Ntot, D] fp64 with bias column, y: [Ntot] (+1/-1); peer p samples B rows of
// [off[p], off[p]+n[p]).  delta = -alpha * g + noise_at_source;  g = X^T(-y/(1+e^{yXw}))/B + lam*w
// noise = (-alpha/B) * sigma*sqrt(B) * N(0,1)  (getNoise: samples are sums over the batch axis)
// =====================================================================================
extern "C" __global__ void __launch_bounds__(64) k_logreg_step(
    const double* X, const double* y, const long long* off, const int* nrows, const int* pid, const double* W, int D,
    int B, int P, unsigned long long seed, const int* calls, double alpha, double lammy, const double* sigma, double qscale,
    float* delta, long long* qdelta) {
  const int p = blockIdx.x;
  if (p >= P) return;
  const int lane = threadIdx.x;
  __shared__ int bidx[64];
  __shared__ double res[64];
  const int n = nrows[p];
  if (lane == 0) {
    int cnt = 0;
    uint32_t ctr = 0;
    while (cnt < B && cnt < n) {
      u4 r = philox(u4{(uint32_t)pid[p], (uint32_t)calls[p], ctr++, 0x106u}, (uint32_t)seed, (uint32_t)(seed >> 32));
      const uint32_t cand[4] = {r.x, r.y, r.z, r.w};
      for (int q = 0; q < 4 && cnt < B && cnt < n; ++q) {
        const int c = (int)(cand[q] % (uint32_t)n);
        bool dup = false;
        for (int t = 0; t < cnt; ++t) dup |= bidx[t] == c;
        if (!dup) bidx[cnt++] = c;
      }
    }
  }
  __syncthreads();
  const int Bq = min(B, n);
  if (lane < Bq) {
    const double* xr = X + (off[p] + bidx[lane]) * (long long)D;
    double z = 0.0;
    for (int k = 0; k < D; ++k) z += xr[k] * W[k];
    const double yy = y[off[p] + bidx[lane]];
    // -y / exp(logaddexp(0, y*z)) == -y / (1 + exp(y*z))
    const double t = yy * z;
    const double lae = t > 0 ? t + log1p(exp(-t)) : log1p(exp(t));
    res[lane] = -yy / exp(lae);
  }
  __syncthreads();
  for (int k = lane; k < D; k += 64) {
    double g = 0.0;
    for (int s = 0; s < Bq; ++s) g += X[(off[p] + bidx[s]) * (long long)D + k] * res[s];
    g = g / (double)B + lammy * W[k];
    double v = -alpha * g;
    if (sigma[p] > 0.0) {
      u4 r = philox(u4{(uint32_t)k, (uint32_t)(calls[p] % 100), (uint32_t)pid[p], 0xD9u}, (uint32_t)(seed >> 7),
                    (uint32_t)(seed >> 39));
      v += (-alpha / (double)B) * sigma[p] * sqrt((double)B) * (double)gauss(r.x, r.y);
    }
    delta[(size_t)p * D + k] = (float)v;
    qdelta[(size_t)p * D + k] = (long long)(v * qscale);
  }
}

// =====================================================================================
// K4: DP noise.  noised[p][i] = delta[p][i] + (1/nn) sum_j scale[j] * N(0,1; key=(seed,noiser_j),
// ctr=(i, it%100)).  A noiser's vector depends only on (noiser, iteration % 100), like the
// reference's pre-sampled samples[it % 100] (client_obj.py:61-63,97-98).
// scale[j] = -sigma_j / sqrt(B)  (sigma_j = 0 for colluding noisers that pre-sampled with eps = 0)
// =====================================================================================
extern "C" __global__ void k_dp_noise(const float* delta, int P, int D, const int* noisers, int nn,
                                      const float* noiser_scale, unsigned long long seed, int iter_mod,
                                      float* noised) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)P * D) return;
  const int p = (int)(g / D), i = (int)(g % D);
  float acc = 0.f;
  for (int j = 0; j < nn; ++j) {
    const int nid = noisers[p * nn + j];
    u4 r = philox(u4{(uint32_t)i, (uint32_t)iter_mod, (uint32_t)nid, 0xA11CEu}, (uint32_t)seed, (uint32_t)(seed >> 32));
    acc += noiser_scale[p * nn + j] * gauss(r.x, r.y);
  }
  noised[g] = delta[g] + (nn > 0 ? acc / (float)nn : 0.f);
}

// K4, resident form.  The reference pre-samples each peer's 100 noise vectors at init
// (samples[it % 100], client_obj.py:61-63); here the whole federation's table [N][100][D]
// (314 MB for MNIST, 100 peers) is built once in HBM with the same Philox counters, and the
// per-round kernel becomes a gather + average (memory-bound) instead of ~2 Philox + Box-Muller
// evaluations per element on the critical path.  Values and float operations are those of
// k_dp_noise, so both forms give identical bits.
extern "C" __global__ void k_noise_table(int nnoisers, int D, unsigned long long seed, float* tbl) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)nnoisers * 100 * D) return;
  const int i = (int)(g % D);
  const long long nm = g / D;
  const int m = (int)(nm % 100), nid = (int)(nm / 100);
  u4 r = philox(u4{(uint32_t)i, (uint32_t)m, (uint32_t)nid, 0xA11CEu}, (uint32_t)seed, (uint32_t)(seed >> 32));
  tbl[g] = gauss(r.x, r.y);
}

// rows (optional): output row p is worker rows[p] -- the verifiers' inbox gathered in arrival order
// straight out of the noise kernel (no separate index_select pass over [n, D])
extern "C" __global__ void k_dp_noise_tbl(const float* delta, int P, int D, const int* noisers, int nn,
                                          const float* noiser_scale, const float* tbl, int iter_mod,
                                          const int* rows, float* noised) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)P * D) return;
  const int p = (int)(g / D), i = (int)(g % D);
  const int src = rows ? rows[p] : p;
  float acc = 0.f;
  for (int j = 0; j < nn; ++j) {
    const int nid = noisers[src * nn + j];
    acc += noiser_scale[src * nn + j] * tbl[((size_t)nid * 100 + iter_mod) * D + i];
  }
  noised[g] = delta[(size_t)src * D + i] + (nn > 0 ? acc / (float)nn : 0.f);
}

// =====================================================================================
// K5a: Gram partials G_part[split][i][j] = sum_{k in split} X[i][k] X[j][k] in f64 via
// v_mfma_f64_16x16x4f64.  Grid (tiles_i, tiles_j, splits), one wave per block.
// f64 16x16x4 layout: A[i=l&15][k=l>>4], B[k=l>>4][j=l&15]; D: col=l&15, row=(l>>4)+4*r.
// =====================================================================================
extern "C" __global__ void __launch_bounds__(64) k_gram_f64(const float* X, int n, int D, int ksplit,
                                                           double* part) {
  const int ti = blockIdx.x, tj = blockIdx.y, sp = blockIdx.z;
  const int lane = threadIdx.x;
  const int i = ti * 16 + (lane & 15), j = tj * 16 + (lane & 15), kk = lane >> 4;
  const int k0 = sp * ksplit, k1 = min(D, k0 + ksplit);
  const float* xa = X + (size_t)min(i, n - 1) * D;
  const float* xb = X + (size_t)min(j, n - 1) * D;
  const bool va = i < n, vb = j < n;
  // loads issued 8 k-steps ahead of the MFMAs, two accumulators (one wave per block, so the
  // memory latency is otherwise fully exposed at every step)
  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  int k = k0;
  for (; k + 32 <= k1; k += 32) {
    float a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      a[u] = xa[k + 4 * u + kk];
      b[u] = xb[k + 4 * u + kk];
    }
#pragma unroll
    for (int u = 0; u < 8; u += 2) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va ? (double)a[u] : 0.0, vb ? (double)b[u] : 0.0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va ? (double)a[u + 1] : 0.0, vb ? (double)b[u + 1] : 0.0, acc1,
                                                  0, 0, 0);
    }
  }
  for (; k < k1; k += 4) {
    const int kx = k + kk;
    const double a = (va && kx < k1) ? (double)xa[kx] : 0.0;
    const double b = (vb && kx < k1) ? (double)xb[kx] : 0.0;
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc0, 0, 0, 0);
  }
  const f64x4 acc = acc0 + acc1;
  const int npad = gridDim.x * 16;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = ti * 16 + (lane >> 4) + 4 * r, col = tj * 16 + (lane & 15);
    part[((size_t)sp * npad + row) * npad + col] = acc[r];
  }
}

// K5b: Krum scores, one wave per row i (n blocks): reduce the split-K Gram partials of row i and of
// the diagonal, D_ij = G_ii + G_jj - 2 G_ij, then score_i = sum of D_ij whose rank in row i lies in
// [1, groupsize-2] -- the sum of the groupsize-2 nearest neighbours after the zero self-distance
// (sort(D_i)[1:groupsize-1], client_obj.py:114-143).  Ranks by parallel counting, ties broken by
// column index; the kept distances are summed in column order (bit-reproducible).  n <= 128.
extern "C" __global__ void __launch_bounds__(64) k_krum_scores(const double* part, int nsplit, int n, int npad,
                                                              int groupsize, double* dist, double* scores) {
  __shared__ double row[128];
  __shared__ double kept[128];
  const int i = blockIdx.x, lane = threadIdx.x;
  double gii = 0.0;
#pragma unroll 8
  for (int s = 0; s < nsplit; ++s) gii += part[((size_t)s * npad + i) * npad + i];
  for (int j = lane; j < n; j += 64) {
    double gij = 0.0, gjj = 0.0;
#pragma unroll 8
    for (int s = 0; s < nsplit; ++s) {
      gij += part[((size_t)s * npad + i) * npad + j];
      gjj += part[((size_t)s * npad + j) * npad + j];
    }
    const double d = gii + gjj - 2.0 * gij;
    row[j] = d;
    dist[(size_t)i * n + j] = d;
  }
  __syncthreads();
  for (int j = lane; j < n; j += 64) {
    const double v = row[j];
    int rank = 0;
    for (int k = 0; k < n; ++k) {
      const double u = row[k];
      rank += (u < v) || (u == v && k < j);
    }
    kept[j] = (rank >= 1 && rank < groupsize - 1) ? v : 0.0;
  }
  __syncthreads();
  if (lane == 0) {
    double a = 0.0;
    for (int j = 0; j < n; ++j) a += kept[j];
    scores[i] = a;
  }
}

// K5c: Multi-Krum selection: accept the n_accept lowest scores (index tiebreak).  One block.
extern "C" __global__ void __launch_bounds__(128) k_krum_accept(const double* scores, int n, int n_accept,
                                                               int* accept) {
  __shared__ double sc[128];
  const int t = threadIdx.x;
  if (t < n) sc[t] = scores[t];
  __syncthreads();
  if (t < n) {
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (sc[j] < sc[t]) || (sc[j] == sc[t] && j < t);
    accept[t] = rank < n_accept ? 1 : 0;
  }
}

// =====================================================================================
// K5 committee form: every verifier runs Multi-Krum on ITS OWN inbox (krum.go:284-322 runs in each
// verifier process over the first KRUM_UPDATETHRESH updates that process received), and an update
// is approved with >= floor(nv/2) signatures (main.go:1686); the leader then builds its block from
// the first NUM_SAMPLES/2 approved arrivals (main.go:360).  All inboxes are subsets of one row set
// X [U, D] (the submitted workers' noised deltas), so the Gram matrix is computed ONCE over X and
// each verifier's distances are gathered out of it:
//   KC1 k_gram_pairs     upper-triangular 16x16 tile pairs x K splits, f64 MFMA, 4 waves per block
//                        split K further and reduce through LDS -> part[split][pair][16][16]
//   KC2 k_krum_rows      one block per (inbox row, verifier): D_ij from the (deterministically
//                        reduced) Gram, rank-select of the groupsize-2 nearest neighbours, score
//                        (krum_rows_body; k_krum_rows_noise / _ka are the same body on another inner product)
//   KC3 k_krum_vote      one block: per-verifier selection of the n_accept lowest scores, signature
//                        count per worker row, approval (>= need), leader cap by arrival rank
// Limits: U <= 1024 rows, inbox n <= 256 on this path; larger committees take the *_big kernels below.
// =====================================================================================
namespace {
__device__ __forceinline__ int pair_index(int ti, int tj, int T) {
  // row-major enumeration of the upper triangle ti <= tj of a T x T tile grid
  return ti * T - (ti * (ti - 1)) / 2 + (tj - ti);
}
// Gram entry G[a][b] out of the reduced upper-triangular tiles
__device__ __forceinline__ double gram_at(const double* gram, int T, int a, int b) {
  int ta = a >> 4, tb = b >> 4, ra = a & 15, rb = b & 15;
  if (ta > tb) {
    const int t = ta; ta = tb; tb = t;
    const int r = ra; ra = rb; rb = r;
  }
  return gram[(size_t)pair_index(ta, tb, T) * 256 + ra * 16 + rb];
}
}  // namespace

// rows [0, U1) of the Gram's operand come from X (row stride D), rows [U1, U) from X2 (row stride
// stride2): the committee Krum's noise-aware form stacks the workers' deltas over the noisers'
// pre-sampled vectors of this iteration (a strided view of the resident noise table)
extern "C" __global__ void __launch_bounds__(256) k_gram_pairs(const float* X, int U, int D, int kchunk, int T,
                                                              double* part, double* gram, unsigned int* count,
                                                              const float* X2, int U1, long long stride2, int pair0,
                                                              const double* nn, int tn0) {
  // high: at priority 1 the pre-step's commitment MSM squeezed it to ~220 us, and its resident workgroups kept
  // the speculative share MSM from being dispatched until it ended (docs/PERF.md round 5); its work is ~10 us
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  __shared__ double red[4][256];
  // this launch covers the tile pairs [pair0, pair0 + gridDim.x) (several ranks split one Gram); part and
  // the arrival counters are indexed by the launch-local pair index, gram by the global one
  const int lp = blockIdx.x, pair = pair0 + lp, sp = blockIdx.y;
  const int npairs = gridDim.x;
  // decode the pair index (T <= 64: a short scan)
  int ti = 0, rem = pair;
  while (rem >= T - ti) {
    rem -= T - ti;
    ++ti;
  }
  const int tj = ti + rem;
  if (nn != nullptr && ti >= tn0) {
    // both tiles hold noise rows only (rows >= U1): the noisers' pre-sampled vectors repeat with the iteration
    // modulo 100 (client_obj.py:61-63,97-98), so this block of the Gram was computed at setup, by this kernel
    // (bit-identical entries), into the dense [U2, U2] table nn of this iteration: copy, no split-K
    if (sp == 0) {
      const int U2 = U - U1, e = threadIdx.x;
      const int a = ti * 16 + (e >> 4) - U1, b = tj * 16 + (e & 15) - U1;
      gram[(size_t)pair * 256 + e] = (a < U2 && b < U2) ? nn[(size_t)a * U2 + b] : 0.0;
    }
    return;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int i = ti * 16 + (lane & 15), j = tj * 16 + (lane & 15), kk = lane >> 4;
  const bool va = i < U, vb = j < U;
  const int ia = va ? i : 0, jb = vb ? j : 0;
  const float* xa = ia < U1 ? X + (size_t)ia * D : X2 + (size_t)(ia - U1) * stride2;
  const float* xb = jb < U1 ? X + (size_t)jb * D : X2 + (size_t)(jb - U1) * stride2;
  // this block's K range, split into 4 wave ranges that are multiples of 4
  const int k0b = sp * kchunk, k1b = min(D, k0b + kchunk);
  const int per = (((k1b - k0b) + 15) / 16) * 4;
  int k = k0b + wid * per;
  const int kend = min(k1b, k + per);
  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  // 32 k per step: lane (r, kk) reads k + 16h + 4kk .. +3 of its row as ONE 16-byte load per half h
  // (4 vector loads per step instead of 16 dword loads); MFMA step (h, c) then sums the elements
  // k + 16h + 4kk + c over kk -- the same k set for A and B, only the summation order differs
  typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
  for (; k + 32 <= kend; k += 32) {
    const f32x4u a0 = *(const f32x4u*)(xa + k + 4 * kk), a1 = *(const f32x4u*)(xa + k + 16 + 4 * kk);
    const f32x4u b0 = *(const f32x4u*)(xb + k + 4 * kk), b1 = *(const f32x4u*)(xb + k + 16 + 4 * kk);
#pragma unroll
    for (int c = 0; c < 4; c += 2) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va ? (double)a0[c] : 0.0, vb ? (double)b0[c] : 0.0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va ? (double)a0[c + 1] : 0.0, vb ? (double)b0[c + 1] : 0.0, acc1,
                                                  0, 0, 0);
    }
#pragma unroll
    for (int c = 0; c < 4; c += 2) {
      acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(va ? (double)a1[c] : 0.0, vb ? (double)b1[c] : 0.0, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(va ? (double)a1[c + 1] : 0.0, vb ? (double)b1[c + 1] : 0.0, acc1,
                                                  0, 0, 0);
    }
  }
  for (; k < kend; k += 4) {
    const int kx = k + kk;
    const double a = (va && kx < kend) ? (double)xa[kx] : 0.0;
    const double b = (vb && kx < kend) ? (double)xb[kx] : 0.0;
    acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc0, 0, 0, 0);
  }
  const f64x4 acc = acc0 + acc1;
  // D layout: lane l holds D[row (l>>4) + 4r][col l&15]
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wid][((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];
  __syncthreads();
  const int e = threadIdx.x;  // 256 threads = the 16x16 tile
  part[((size_t)sp * npairs + lp) * 256 + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
  // the split-K partials are summed by k_gram_reduce (the next launch on the stream).  An in-kernel
  // last-block reduction needed an agent-scope release / acquire per block: on gfx950 that is an L2
  // write-back + invalidate (buffer_wbl2 / buffer_inv sc1) in each of the ~1450 blocks -- ~100 us for ~10 us of
  // MFMA work, and every kernel beside it (the share MSMs' table lookups) lost its L2 lines too
}

// KC1b: tile pair p's reduced Gram tile = sum of its split-K partials in split order (bit-reproducible, the
// same order as before); the noise-only tile pairs were copied from the table by k_gram_pairs (split 0)
extern "C" __global__ void __launch_bounds__(256) k_gram_reduce(const double* part, double* gram, int npairs,
                                                               int nsplit, int pair0, int T, int tn0, int has_nn) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  const int lp = blockIdx.x, pair = pair0 + lp, e = threadIdx.x;
  if (has_nn) {
    int ti = 0, rem = pair;
    while (rem >= T - ti) {
      rem -= T - ti;
      ++ti;
    }
    if (ti >= tn0) return;   // noise x noise: already in place
  }
  double g = 0.0;
  for (int q = 0; q < nsplit; ++q) g += part[((size_t)q * npairs + lp) * 256 + e];
  gram[(size_t)pair * 256 + e] = g;
}

// KC2, noise-aware form: the candidate rows are x_a = delta_a + (1/nn) sum_s sc[a][s] t_{nz[a][s]}
// (the noisers' pre-sampled vectors, main.go:1592-1660), and the Gram was taken over the stacked
// [deltas; noise vectors] rows, so <x_a, x_b> expands into (1 + nn)^2 Gram entries -- the
// d-dimensional work (the Gram) runs before the noisers are known (they come from the workers' VRF
// outputs on the host); only this O(n^2 nn^2) assembly waits for them.
namespace {
// the noisers' ids and weights: device arrays, or (NoiseArg) the kernel's argument block -- the round's tables
// are ~1.6 KB at 100 peers, so they ride in the launch instead of an upload copy the selection queues behind
#define NOISE_ARG_MAX 400
struct NoiseArg {
  int nz[NOISE_ARG_MAX];
  float sc[NOISE_ARG_MAX];
};
struct NoisePtr {
  const int* z;
  const float* s;
  __device__ __forceinline__ int nz(int i) const { return z[i]; }
  __device__ __forceinline__ float sc(int i) const { return s[i]; }
};
struct NoiseByVal {
  const NoiseArg* a;
  __device__ __forceinline__ int nz(int i) const { return a->nz[i]; }
  __device__ __forceinline__ float sc(int i) const { return a->sc[i]; }
};

template <class N>
__device__ __forceinline__ double xx_dot(const double* gram, int T, int U1, N q, int nn, int a, int b) {
  double v = gram_at(gram, T, a, b);
  const double inv = 1.0 / (double)nn;
  for (int t = 0; t < nn; ++t) {
    v += inv * (double)q.sc(b * nn + t) * gram_at(gram, T, a, U1 + q.nz(b * nn + t));
    v += inv * (double)q.sc(a * nn + t) * gram_at(gram, T, U1 + q.nz(a * nn + t), b);
  }
  for (int s2 = 0; s2 < nn; ++s2)
    for (int t = 0; t < nn; ++t)
      v += inv * inv * (double)q.sc(a * nn + s2) * (double)q.sc(b * nn + t) *
           gram_at(gram, T, U1 + q.nz(a * nn + s2), U1 + q.nz(b * nn + t));
  return v;
}

// the inner product <x_a, x_b> of two candidate rows, in its two forms: a Gram entry, or the noise-aware assembly
struct PlainDot {
  const double* gram;
  int T;
  __device__ __forceinline__ double operator()(int a, int b) const { return gram_at(gram, T, a, b); }
};
template <class N>
struct NoiseDot {
  const double* gram;
  int T, U1;
  N q;
  int nn;
  __device__ __forceinline__ double operator()(int a, int b) const { return xx_dot(gram, T, U1, q, nn, a, b); }
};

// KC2, every form: block (i, v) scores row i of verifier v's inbox.  Thread t holds the squared distance
// <a,a> + <b,b> - 2 <a,b> to inbox row t (<a,a> once per block), ranks it among the row's distances (index
// tie-break) and keeps it when 1 <= rank < groupsize - 1; thread 0 sums the kept values serially in inbox order
// (the f64 summation order the accept masks depend on)
template <class Dot>
__device__ __forceinline__ void krum_rows_body(Dot dot, const int* inbox, int n, int groupsize, double* scores) {
  __shared__ double row[256];
  __shared__ double kept[256];
  __shared__ double xaa;
  const int i = blockIdx.x, v = blockIdx.y, t = threadIdx.x;
  const int* box = inbox + (size_t)v * n;
  const int a = box[i];
  if (t == 0) xaa = dot(a, a);
  __syncthreads();
  if (t < n) {
    const int b = box[t];
    row[t] = xaa + dot(b, b) - 2.0 * dot(a, b);
  }
  __syncthreads();
  if (t < n) {
    const double val = row[t];
    int rank = 0;
    for (int k2 = 0; k2 < n; ++k2) {
      const double u = row[k2];
      rank += (u < val) || (u == val && k2 < t);
    }
    kept[t] = (rank >= 1 && rank < groupsize - 1) ? val : 0.0;
  }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += kept[j];
    scores[(size_t)v * n + i] = s;
  }
}
}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_krum_rows(const double* gram, int T, const int* inbox, int n,
                                                             int groupsize, double* scores) {
  krum_rows_body(PlainDot{gram, T}, inbox, n, groupsize, scores);
}

// the noise forms run beside the share MSMs, with the round waiting on them: high wave priority
extern "C" __global__ void __launch_bounds__(256) k_krum_rows_noise(const double* gram, int T, int U1,
                                                                   const int* nz, const float* sc, int nn,
                                                                   const int* inbox, int n, int groupsize,
                                                                   double* scores) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  krum_rows_body(NoiseDot<NoisePtr>{gram, T, U1, {nz, sc}, nn}, inbox, n, groupsize, scores);
}

extern "C" __global__ void __launch_bounds__(256) k_krum_rows_noise_ka(const double* gram, int T, int U1, NoiseArg q,
                                                                      int nn, const int* inbox, int n, int groupsize,
                                                                      double* scores) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  krum_rows_body(NoiseDot<NoiseByVal>{gram, T, U1, {&q}, nn}, inbox, n, groupsize, scores);
}

// h_acc / h_node (nullable): the same verdicts written straight into pinned host memory (the host reads them
// after the kernel's event: no read-back copy); amap / alive / nspec (nullable): the speculative share MSM's
// row flags set from the block mask (k_set_alive fused: alive[i] = node[amap[i]], 0 where amap[i] < 0)
extern "C" __global__ void __launch_bounds__(1024) k_krum_vote(const double* scores, const int* inbox, int V, int n,
                                                              int n_accept, int U, int need, const int* lead_rank,
                                                              int cap, int* acc, int* node, int* h_acc, int* h_node,
                                                              const int* amap, int nspec, int* alive) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  __shared__ int sigs[1024];
  __shared__ int appr[1024];
  __shared__ int lr[1024];
  __shared__ int kept[1024];
  __shared__ double sv[4][256];
  const int t = threadIdx.x;
  for (int w = t; w < U; w += 1024) {
    sigs[w] = 0;
    lr[w] = lead_rank[w];
  }
  // per-verifier Multi-Krum selection: the n_accept lowest scores (index tie-break); four verifiers
  // at a time, their scores staged in LDS
  for (int v0 = 0; v0 < V; v0 += 4) {
    const int nv = min(4, V - v0);
    __syncthreads();
    for (int e = t; e < nv * n; e += 1024) sv[e / n][e % n] = scores[(size_t)(v0 + e / n) * n + e % n];
    __syncthreads();
    for (int e = t; e < nv * n; e += 1024) {
      const int vv = e / n, i = e % n;
      const double s = sv[vv][i];
      int rank = 0;
      for (int j = 0; j < n; ++j) rank += (sv[vv][j] < s) || (sv[vv][j] == s && j < i);
      const int ok = rank < n_accept ? 1 : 0;
      const size_t ge = (size_t)(v0 + vv) * n + i;
      acc[ge] = ok;
      if (h_acc != nullptr) h_acc[ge] = ok;
      if (ok) atomicAdd(&sigs[inbox[ge]], 1);
    }
  }
  __syncthreads();
  // approval: >= need signatures among the submitted workers (lead_rank >= 0)
  for (int w = t; w < U; w += 1024) appr[w] = (lr[w] >= 0 && sigs[w] >= need) ? 1 : 0;
  __syncthreads();
  // the leader's block: the first `cap` approved rows in leader arrival order (cap <= 0: all)
  for (int w = t; w < U; w += 1024) {
    int keep = appr[w];
    if (keep && cap > 0) {
      int before = 0;
      const int r = lr[w];
      for (int x = 0; x < U; ++x) before += appr[x] && lr[x] < r;
      keep = before < cap;
    }
    node[w] = keep;
    kept[w] = keep;
    if (h_node != nullptr) h_node[w] = keep;
  }
  if (alive != nullptr) {
    __syncthreads();
    for (int i = t; i < nspec; i += 1024) {
      const int j = amap[i];
      __hip_atomic_store(alive + i, (j >= 0 && j < U && kept[j]) ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (h_acc != nullptr || h_node != nullptr) __threadfence_system();
}

// ---- large committees (an inbox of more than 256 updates, or more than 1024 candidate rows): the
// reference's Krum has no size limit (client_obj.py:114-143).  A row's distances are sorted in LDS
// (bitonic) and its score is the sum of the sorted values at positions 1 .. groupsize-2 -- the same
// multiset as k_krum_rows' rank select (ties cannot change it); the vote counts signatures in a global
// workspace and the leader cap runs one thread per candidate row.  Limits: U <= 8192, n <= 4096.
namespace {
__device__ void bitonic_sort_lds(double* a, int npow2) {
  for (int k = 2; k <= npow2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < npow2; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const bool up = (i & k) == 0;
          const double x = a[i], y = a[ixj];
          if ((x > y) == up) {
            a[i] = y;
            a[ixj] = x;
          }
        }
      }
      __syncthreads();
    }
}
}  // namespace

template <class Dot>
__global__ void __launch_bounds__(1024) k_krum_rows_big(Dot dot, const int* inbox, int n, int npow2, int groupsize,
                                                        double* scores) {
  extern __shared__ double row[];   // [npow2]
  __shared__ double xaa;
  const int i = blockIdx.x, v = blockIdx.y;
  const int* box = inbox + (size_t)v * n;
  const int a = box[i];
  if (threadIdx.x == 0) xaa = dot(a, a);
  __syncthreads();
  for (int t = threadIdx.x; t < npow2; t += blockDim.x) {
    double val = __builtin_huge_val();
    if (t < n) {
      const int b = box[t];
      val = xaa + dot(b, b) - 2.0 * dot(a, b);
    }
    row[t] = val;
  }
  __syncthreads();
  bitonic_sort_lds(row, npow2);
  if (threadIdx.x == 0) {
    double s = 0.0;
    const int hi = min(groupsize - 1, n);
    for (int j = 1; j < hi; ++j) s += row[j];
    scores[(size_t)v * n + i] = s;
  }
}

// per-verifier selection (one block per verifier): the n_accept lowest scores, index tie-break; the
// signatures each candidate row collects go to `sigs` (zeroed by the launcher)
extern "C" __global__ void __launch_bounds__(1024) k_krum_select_big(const double* scores, const int* inbox, int n,
                                                                    int n_accept, int* acc, int* sigs) {
  extern __shared__ double sv[];   // [n]
  const int v = blockIdx.x;
  for (int e = threadIdx.x; e < n; e += blockDim.x) sv[e] = scores[(size_t)v * n + e];
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const double s = sv[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += (sv[j] < s) || (sv[j] == s && j < i);
    const int ok = rank < n_accept ? 1 : 0;
    acc[(size_t)v * n + i] = ok;
    if (ok) atomicAdd(&sigs[inbox[(size_t)v * n + i]], 1);
  }
}

// approval (>= need signatures, submitted) and the leader's cap: the first `cap` approved rows in
// leader arrival order (cap <= 0: all); one thread per candidate row
extern "C" __global__ void __launch_bounds__(256) k_krum_cap_big(const int* sigs, const int* lead_rank, int U,
                                                                int need, int cap, int* node) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= U) return;
  const int lr = lead_rank[w];
  int keep = (lr >= 0 && sigs[w] >= need) ? 1 : 0;
  if (keep && cap > 0) {
    int before = 0;
    for (int x = 0; x < U; ++x) before += (lead_rank[x] >= 0 && sigs[x] >= need && lead_rank[x] < lr) ? 1 : 0;
    keep = before < cap;
  }
  node[w] = keep;
}

namespace {
int krum_vote_any(hipStream_t s, const double* scores, const int* inbox, int V, int n, int n_accept, int U, int need,
                  const int* lead_rank, int cap, int* acc, int* node, int* ws, int* h_out = nullptr,
                  const int* amap = nullptr, int nspec = 0, int* alive = nullptr) {
  if (U <= 1024 && n <= 256) {
    hipLaunchKernelGGL(k_krum_vote, dim3(1), dim3(1024), 0, s, scores, inbox, V, n, n_accept, U, need, lead_rank,
                       cap, acc, node, h_out, h_out != nullptr ? h_out + (size_t)V * n : nullptr, amap, nspec, alive);
  } else {
    if (ws == nullptr) return -1;
    if (hipMemsetAsync(ws, 0, (size_t)U * sizeof(int), s) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_krum_select_big, dim3(V), dim3(1024), (size_t)n * sizeof(double), s, scores, inbox, n,
                       n_accept, acc, ws);
    hipLaunchKernelGGL(k_krum_cap_big, dim3((U + 255) / 256), dim3(256), 0, s, (const int*)ws, lead_rank, U, need, cap,
                       node);
    // large committees: the read-back copy and the flag update stay separate launches
    if (h_out != nullptr && hipMemcpyAsync(h_out, acc, ((size_t)V * n + U) * sizeof(int), hipMemcpyDeviceToHost, s) !=
                                hipSuccess)
      return -1;
    if (alive != nullptr && nspec > 0 && bsc_set_alive(node, amap, nspec, alive, s) != 0) return -1;
  }
  return 0;
}
int pow2_at_least(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}
}  // namespace

// =====================================================================================
// LSH sieve (ML/code/logistic_aggregator.py:7-29, the third poisoning defence next to Krum and RONI):
// every update's weight is 1 / #(its near neighbours within squared distance thr among the
// (centred) updates), so a cluster of sybil updates shares the weight of one.  The reference asks a
// FALCONN index (random-projection LSH) for the neighbours; here:
//   LS1 k_lsh_codes    L tables x K sign bits of <x_i - mu, r> per row (one block per row)
//   LS2 k_lsh_count    neighbour count of each listed row: candidates share a bucket in some table
//                      (L = 0: every pair, the exact query), confirmed on the f64 Gram (KC1 tiles;
//                      centring cancels in differences)
//   LS3 k_weighted_rows  out = sum_i w_i x_i in fp64
// =====================================================================================
extern "C" __global__ void __launch_bounds__(256) k_lsh_codes(const float* X, const float* mu, int n, int D,
                                                             const float* planes, int L, int K,
                                                             unsigned int* codes) {
  __shared__ float red[4][64];
  const int i = blockIdx.x, t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const int P = L * K;   // <= 64 planes
  float acc[64];
#pragma unroll
  for (int q = 0; q < 64; ++q) acc[q] = 0.f;
  for (int k = t; k < D; k += 256) {
    const float v = X[(size_t)i * D + k] - mu[k];
#pragma unroll
    for (int q = 0; q < 64; ++q)
      if (q < P) acc[q] += v * planes[(size_t)q * D + k];
  }
#pragma unroll
  for (int q = 0; q < 64; ++q) {
    float v = acc[q];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) red[wid][q] = v;
  }
  __syncthreads();
  if (t < L) {
    unsigned int c = 0;
    for (int b = 0; b < K; ++b) {
      const int q = t * K + b;
      const float v = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
      c |= (v > 0.f ? 1u : 0u) << b;
    }
    codes[(size_t)i * L + t] = c;
  }
}

extern "C" __global__ void __launch_bounds__(256) k_lsh_count(const double* gram, int T, const unsigned int* codes,
                                                             int L, const int* rows, int m, double thr, int* counts) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= m) return;
  const int i = rows[a];
  const double gii = gram_at(gram, T, i, i);
  int c = 0;
  for (int b = 0; b < m; ++b) {
    const int j = rows[b];
    bool cand = L == 0 || j == i;
    for (int tb = 0; tb < L && !cand; ++tb) cand = codes[(size_t)i * L + tb] == codes[(size_t)j * L + tb];
    if (!cand) continue;
    const double d2 = gii + gram_at(gram, T, j, j) - 2.0 * gram_at(gram, T, i, j);
    c += (j == i || d2 < thr) ? 1 : 0;
  }
  counts[a] = c;
}

extern "C" __global__ void k_weighted_rows(const float* X, int n, int D, const double* w, double* out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= D) return;
  double acc = 0.0;
  for (int i = 0; i < n; ++i) acc += w[i] * (double)X[(size_t)i * D + k];
  out[k] = acc;
}

extern "C" int bsc_lsh_codes(const float* X, const float* mu, int n, int D, const float* planes, int L, int K,
                             unsigned int* codes, void* stream) {
  if (n <= 0 || L <= 0) return 0;
  if (L * K > 64 || K > 32 || K <= 0) return -1;
  hipLaunchKernelGGL(k_lsh_codes, dim3(n), dim3(256), 0, (hipStream_t)stream, X, mu, n, D, planes, L, K, codes);
  return (int)hipGetLastError();
}
extern "C" int bsc_lsh_count(const double* gram, int U, const unsigned int* codes, int L, const int* rows, int m,
                             double thr, int* counts, void* stream) {
  if (m <= 0) return 0;
  const int T = (U + 15) / 16;
  hipLaunchKernelGGL(k_lsh_count, dim3((m + 255) / 256), dim3(256), 0, (hipStream_t)stream, gram, T, codes, L, rows, m,
                     thr, counts);
  return (int)hipGetLastError();
}
extern "C" int bsc_weighted_rows(const float* X, int n, int D, const double* w, double* out, void* stream) {
  if (D <= 0) return 0;
  hipLaunchKernelGGL(k_weighted_rows, dim3((D + 255) / 256), dim3(256), 0, (hipStream_t)stream, X, n, D, w, out);
  return (int)hipGetLastError();
}

// =====================================================================================
// K2: softmax scoring of 16-row tiles, shared by k_eval_error, k_eval_error_t and k_roni_counts.
// One block per tile: logits = A_tile[16 x D_IN] . B^T on v_mfma_f32_16x16x4f32 (lane l holds
// A[row l&15][k l>>4] and B[k l>>4][class l&15]).  The 4 waves split K; each runs 8 k-groups (of 4
// features) per step on two accumulators (they hide the 40-cycle dependent latency; loads are issued 8
// k-groups ahead), then a guarded one-group tail on the first accumulator; acc0 + acc1 goes to LDS and wave
// 0 sums the four partials as (0 + 1) + (2 + 3), adds the bias and takes the argmax across the 16 class
// lanes by xor-shuffles (first maximum, like np.argmax).  That order is part of the result: RONI's counts
// equal the evaluation's exactly because both run this one body.
//   A sources: EvalRows  -- row-major rows, (x - tsub) * tmul fused
//              EvalTiles -- cached pre-transformed tiles, one coalesced 256-byte load per k-group
//   B sources: ModelB      -- (float)W[e]
//              ModelPlusB  -- (float)(W[e] + (double)U[c][e]): the sum in fp64, rounded once
// A partial last k-group (D_IN % 4 != 0) is summed where each caller's stop puts it: the row kernels stop at
// the end of the wave's features, so it goes through the tail, into acc0; the tile kernel stops at the end of its
// (padded) k-groups, so it can sit in the unrolled loop and land in acc1.  The two orders differ in the last bits.
// =====================================================================================
namespace {
// A sources: element (lane's row, feature k + kk) of the k-group at k (a multiple of 4)
struct EvalRows {
  static constexpr bool kPadded = false;
  const float* xr;   // this lane's row
  float tsub, tmul;
  int klim;          // end of the wave's K range: nothing is read or summed from there on
  __device__ __forceinline__ float load(int k, int kk) const { return xr[k + kk]; }
  __device__ __forceinline__ float operand(float x) const { return (x - tsub) * tmul; }
};
struct EvalTiles {
  static constexpr bool kPadded = true;   // whole k-groups, zeros past D_IN: loads need no guard
  const float* xp;   // tile base + lane
  int klim;          // D_IN: B is not read from there on
  __device__ __forceinline__ float load(int k, int) const { return xp[(size_t)k * 16]; }
  __device__ __forceinline__ float operand(float x) const { return x; }
};
// the B sources index from where they are pointed: the lane's class row for the logits, the model for the bias
struct ModelB {
  const double* w;
  __device__ __forceinline__ float operator()(int k) const { return (float)w[k]; }
};
struct ModelPlusB {
  const double* w;
  const float* u;   // the candidate update, laid out like the model
  bool upd;
  __device__ __forceinline__ float operator()(int k) const { return upd ? (float)(w[k] + (double)u[k]) : (float)w[k]; }
};

// the tile's logits, as four per-wave partials in red: the wave's k-groups from k0 (a multiple of 4) up to kstop,
// 8 per unrolled step while 32 features remain before kstop, then one at a time.  wb: the B source at this lane's
// class row (cval: the lane has a class).  Returns true in wave 0, which goes on to score; the other waves are done.
template <class A, class B>
__device__ __forceinline__ bool softmax_tile_logits(float (&red)[4][4][64], const A& xa, const B& wb, bool cval,
                                                    int k0, int kstop) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, kk = lane >> 4;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (; k0 + 32 <= kstop; k0 += 32) {
    float a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = k0 + 4 * u + kk;
      a[u] = xa.load(k0 + 4 * u, kk);
      b[u] = (cval && (!A::kPadded || k < xa.klim)) ? wb(k) : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; u += 2) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.operand(a[u]), b[u], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(xa.operand(a[u + 1]), b[u + 1], acc1, 0, 0, 0);
    }
  }
  for (; k0 < kstop; k0 += 4) {
    const int k = k0 + kk;
    const bool in = k < xa.klim;
    const float a = (A::kPadded || in) ? xa.operand(xa.load(k0, kk)) : 0.f;
    const float b = (in && cval) ? wb(k) : 0.f;
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc0, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wid][r][lane] = acc0[r] + acc1[r];
  __syncthreads();
  return wid == 0;
}

// wave 0: the predicted class of tile row (lane >> 4) * 4 + r (the D layout of 16x16x4 f32: lane l holds
// D[row (l>>4)*4 + r][class l&15]), in every lane of the row's 16
__device__ __forceinline__ int softmax_tile_class(const float (&red)[4][4][64], int r, bool cval, float bias) {
  const int lane = threadIdx.x & 63;
  const float logit = (red[0][r][lane] + red[1][r][lane]) + (red[2][r][lane] + red[3][r][lane]);
  float bv = cval ? logit + bias : -__builtin_huge_valf();
  int bc = lane & 15;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 16);
    const int oc = __shfl_xor(bc, o, 16);
    if (ov > bv || (ov == bv && oc < bc)) {
      bv = ov;
      bc = oc;
    }
  }
  return bc;
}

// the evaluation kernels' epilogue: misses over up to two row sets (rows [0, split) and [split, N)), one atomic
// per (wave, set): err[row >= split] += #(argmax != label)
__device__ __forceinline__ void eval_count_sets(const float (&red)[4][4][64], int row0, bool cval, float bias,
                                                const int* y, int N, int split, unsigned int* err) {
  const int lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4;
  unsigned int cnt0 = 0, cnt1 = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int bc = softmax_tile_class(red, r, cval, bias);
    const int row = row0 + kk * 4 + r;
    if (i == 0 && row < N && bc != y[row]) {
      if (row < split) ++cnt0;
      else ++cnt1;
    }
  }
  if (i == 0) {
    if (cnt0) atomicAdd(err, cnt0);
    if (cnt1) atomicAdd(err + 1, cnt1);
  }
}
}  // namespace

// classification error of a softmax model over up to two row sets in ONE launch (test rows [0, split), attack
// rows [split, N)), on row-major X with the (x - 0.5) / 0.5 transform fused
extern "C" __global__ void __launch_bounds__(256) k_eval_error(const float* X, const int* y, int N, int D_IN,
                                                              int D_OUT, const double* W, int transform, int split,
                                                              unsigned int* err) {
  __shared__ float red[4][4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int row0 = blockIdx.x * 16;
  const int i = lane & 15;
  const bool cval = i < D_OUT;
  const int kq = ((D_IN + 15) / 16) * 4;  // this wave's K range: multiple of 4
  const int k0 = wid * kq, kend = min(D_IN, k0 + kq);
  const EvalRows xa{X + (size_t)min(row0 + i, N - 1) * D_IN, transform ? 0.5f : 0.f, transform ? 2.f : 1.f, kend};
  const ModelB wb{W + (size_t)(cval ? i : 0) * D_IN};
  if (!softmax_tile_logits(red, xa, wb, cval, k0, kend)) return;
  const float bias = cval ? ModelB{W}(D_OUT * D_IN + i) : 0.f;
  eval_count_sets(red, row0, cval, bias, y, N, split, err);
}

// The same on a cached, pre-transformed test set: Xt[tile][g][64] holds (x - 0.5) / 0.5 of row
// tile*16 + (l & 15), feature 4g + (l >> 4) for lane l -- exactly the A operand of one
// v_mfma_f32_16x16x4f32 step -- built once per task (the test rows never change): no row-strided gathers and
// no per-element transform.  Ahead of the share MSM's waves (the evaluation is read one round later and
// must be done by then under that load).
extern "C" __global__ void __launch_bounds__(256) k_eval_error_t(const float* Xt, const int* y, int N, int KG, int D_IN,
                                                                int D_OUT, const double* W, int split,
                                                                unsigned int* err, unsigned int* err_host) {
  BSC_SET_PRIO(BSC_PRIO_AHEAD);
  __shared__ float red[4][4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, tile = blockIdx.x;
  const int i = lane & 15;
  const bool cval = i < D_OUT;
  const int gq = (KG + 3) / 4;   // this wave's k-groups
  const int g0 = wid * gq, gend = min(KG, g0 + gq);
  const EvalTiles xa{Xt + (size_t)tile * KG * 64 + lane, D_IN};
  const ModelB wb{W + (size_t)(cval ? i : 0) * D_IN};
  if (!softmax_tile_logits(red, xa, wb, cval, 4 * g0, 4 * gend)) return;
  const float bias = cval ? ModelB{W}(D_OUT * D_IN + i) : 0.f;
  eval_count_sets(red, tile * 16, cval, bias, y, N, split, err);
  // err_host (bsc_eval_error_t_rb): k_eval_finish, the next launch, hands the counts to the host and re-zeroes
  // them.  (A last-tile hand-off inside this kernel needed an agent-scope fence per wave -- on gfx950 an L2
  // write-back + invalidate, ~625 of them beside the share MSMs.)
  (void)err_host;
}

// the evaluation's two counts into pinned host memory, counters re-zeroed for the next launch: one wave, behind
// k_eval_error_t on its stream (no fill and no copy blit: each waited ~20-40 us for a CU slot behind the MSMs)
extern "C" __global__ void __launch_bounds__(64) k_eval_finish(unsigned int* err, unsigned int* err_host) {
  if (threadIdx.x == 0) {
    err_host[0] = err[0];
    err_host[1] = err[1];
    err[0] = 0u;
    err[1] = 0u;
    err[2] = 0u;
  }
}

// K2m: the same two miss counts for K1m's MLP (W in its layout).  One block per 16-row tile, on the step's forward:
// each feature of the tile's rows is staged once, MLP_KT at a time with the transform fused, the 4 waves split
// the k steps of a staged tile and feed all NCT column tiles; h = relu(Z1 + b1) stays in LDS and wave 0 takes it
// through the second layer (K = H, W2 from L2) to the argmax across the 16 class lanes (first maximum) and the
// compare against y: one integer atomic per (four rows, set) that missed.  LDS: 17664 + 4096 NCT + 64 (H + 1) + 128 bytes.
template <int NCT>
__global__ void __launch_bounds__(256) k_mlp_eval(const float* X, const int* y, int N, int D_IN, int D_OUT,
                                                  const double* W, int transform, int split, unsigned int* err) {
  constexpr int H = NCT * 16;
  __shared__ float xs[16 * MLP_KS];
  __shared__ float red[4][NCT][16][16];
  __shared__ float hs[16][H + 1];
  __shared__ long long rowidx[16];
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 15, kk = lane >> 4;
  const int row0 = blockIdx.x * 16;
  if (tid < 16) rowidx[tid] = row0 + tid < N ? row0 + tid : -1;
  __syncthreads();
  const double *b1 = W + (size_t)H * D_IN, *W2 = b1 + H, *b2 = W2 + D_OUT * H;
  mlp_hidden_partials<NCT, false>(xs, red, nullptr, X, rowidx, W, D_IN, transform ? 0.5f : 0.f, transform ? 2.f : 1.f);
  mlp_hidden_relu<NCT>(red, b1, 16, hs);
  if (tid >= 64) return;
  const bool cval = i < D_OUT;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < H / 4; ++st) {
    const float bv = cval ? (float)W2[i * H + st * 4 + kk] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hs[i][st * 4 + kk], bv, acc, 0, 0, 0);
  }
  const float bias = cval ? (float)b2[i] : 0.f;
  unsigned int cnt0 = 0, cnt1 = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {   // lane holds the logit of row kk * 4 + r, class i
    float bv = cval ? acc[r] + bias : -__builtin_huge_valf();
    int bc = i;
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 16);
      const int oc = __shfl_xor(bc, o, 16);
      if (ov > bv || (ov == bv && oc < bc)) {
        bv = ov;
        bc = oc;
      }
    }
    const int row = row0 + kk * 4 + r;
    if (i == 0 && row < N && bc != y[row]) {
      if (row < split) ++cnt0;
      else ++cnt1;
    }
  }
  if (i == 0) {
    if (cnt0) atomicAdd(err, cnt0);
    if (cnt1) atomicAdd(err + 1, cnt1);
  }
}

// K2c: the same two miss counts for K1c's CNN (W in its layout).  One block per 16 rows on the step's forward body
// (cnn_forward without the Gram): the rows' images staged once with the transform fused, the per-wave partial
// logits combined in LDS in the step's order, then one thread per row takes the argmax (first maximum) and wave 0
// counts the misses of either set by ballot: at most two integer atomics per block.  LDS: K1c's 119872 dynamic bytes
// + 4096 partials + 128.
extern "C" __global__ void __launch_bounds__(256) k_cnn_eval(const float* X, const int* y, int N, int S, int D_OUT,
                                                             const double* W, int transform, int split,
                                                             unsigned int* err) {
  extern __shared__ float cnn_lds[];
  __shared__ float red[4][16][16];
  __shared__ long long rowidx[16];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, i = lane & 15, kk = lane >> 4;
  const int row0 = blockIdx.x * 16, NP = (S + 4) * (S + 4);
  const double *bc = W + 400, *Wfc = W + 416, *bfc = Wfc + (size_t)D_OUT * 16 * NP;
  if (tid < 16) rowidx[tid] = row0 + tid < N ? row0 + tid : -1;
  __syncthreads();
  cnn_stage_images(cnn_lds, X, rowidx, S, (S * S) | 1, transform ? 0.5f : 0.f, transform ? 2.f : 1.f);
  const CnnLane L = cnn_lane(W);
  __syncthreads();
  f32x4 accl = {0.f, 0.f, 0.f, 0.f}, unused = {0.f, 0.f, 0.f, 0.f};
  cnn_forward<false>(cnn_lds, cnn_lds + CNN_IMG + wid * CNN_STAGE, S, Wfc, bc, D_OUT, 16, L, accl, unused);
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wid][kk * 4 + r][i] = accl[r];
  __syncthreads();
  if (tid >= 64) return;
  const int row = row0 + tid;
  bool miss = false;
  if (tid < 16 && row < N) {
    float bv = -__builtin_huge_valf();
    int bcl = 0;
    for (int c = 0; c < D_OUT; ++c) {
      const float v = (red[0][c][tid] + red[1][c][tid]) + (red[2][c][tid] + red[3][c][tid]) + (float)bfc[c];
      if (v > bv) {
        bv = v;
        bcl = c;
      }
    }
    miss = bcl != y[row];
  }
  const unsigned int cnt0 = (unsigned int)__popcll(__ballot(miss && row < split));
  const unsigned int cnt1 = (unsigned int)__popcll(__ballot(miss && row >= split));
  if (tid == 0) {
    if (cnt0) atomicAdd(err, cnt0);
    if (cnt1) atomicAdd(err + 1, cnt1);
  }
}

// =====================================================================================
// Committee RONI (VerifyUpdateRONI, main.go:191-233): every local verifier's minibatch scored under the base
// model and under W + U[c] for every row c of its inbox, in ONE launch.  counts[v][0] = #misclassified
// minibatch rows of verifier v under W; counts[v][1 + j] the same under W + U[cand[v][j]].
// One block per (column, verifier, 16-row tile of the minibatch), on K2's scoring body with k_eval_error's A
// source and the B operand (float)(W[k] + (double)U[c][k]) formed in registers -- what the host loop's
// `W + X[i].double()` followed by k_eval_error's (float)W[k] gives -- so the logits, and with them the counts,
// are bit-identical to one k_eval_error launch per (verifier, candidate).  The minibatch rows are gathered by
// index (rows: absolute rows of X); slots past nrows[v] load a clamped row and are not counted.
// =====================================================================================
extern "C" __global__ void __launch_bounds__(256) k_roni_counts(const float* X, const int* y, long long NX, int D_IN,
                                                               int D_OUT, const double* W, const float* U, int n_cand,
                                                               const long long* rows, const int* nrows, int Bmax,
                                                               const int* cand, int ni, int transform,
                                                               unsigned int* counts) {
  __shared__ float red[4][4][64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int col = blockIdx.x, v = blockIdx.y, row0 = blockIdx.z * 16;
  const int nr = min(nrows[v], Bmax);
  if (row0 >= nr) return;  // the whole block: no barrier is skipped by part of it
  const int i = lane & 15, kk = lane >> 4;
  const long long* rv = rows + (size_t)v * Bmax;
  const long long gr = min(max(rv[min(row0 + i, nr - 1)], 0ll), NX - 1);
  const bool cval = i < D_OUT;
  // column 0 is the base model; an inbox slot without a row (cand < 0 or past U) is scored as the base model
  const int c = col > 0 ? cand[(size_t)v * ni + (col - 1)] : -1;
  const bool upd = c >= 0 && c < n_cand;
  const size_t D = (size_t)D_OUT * D_IN + D_OUT;
  const int kq = ((D_IN + 15) / 16) * 4;  // this wave's K range: multiple of 4
  const int k0 = wid * kq, kend = min(D_IN, k0 + kq);
  const EvalRows xa{X + (size_t)gr * D_IN, transform ? 0.5f : 0.f, transform ? 2.f : 1.f, kend};
  const float* uc = U + (upd ? (size_t)c * D : 0);
  const size_t wo = (size_t)(cval ? i : 0) * D_IN;
  const ModelPlusB wb{W + wo, uc + wo, upd};
  if (!softmax_tile_logits(red, xa, wb, cval, k0, kend)) return;
  const float bias = cval ? ModelPlusB{W, uc, upd}(D_OUT * D_IN + i) : 0.f;
  unsigned int cnt = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int bc = softmax_tile_class(red, r, cval, bias);
    const int row = row0 + kk * 4 + r;
    if (i == 0 && row < nr && bc != y[min(max(rv[row], 0ll), NX - 1)]) ++cnt;
  }
  // the four row groups' counts (lanes 0, 16, 32, 48) into lane 0: one store per block, or one atomic when the
  // minibatch spans several tiles (the counters are zeroed before the launch)
  cnt += __shfl_xor(cnt, 16);
  cnt += __shfl_xor(cnt, 32);
  if (lane == 0) {
    unsigned int* out = counts + (size_t)v * (ni + 1) + col;
    if (Bmax <= 16) *out = cnt;
    else if (cnt) atomicAdd(out, cnt);
  }
}

// =====================================================================================
// Logistic scoring (creditcard: logistic_model.py's sign(X w) != y), for the evaluation and for committee RONI:
// counts[m][s] = #rows of set s (rows [0, split): 0, rows [split, N): 1) with sign(x . w_m) != y, sign(0) = 0
// counting as wrong like torch.sign.  Model 0 is W; model m >= 1 is W[k] + (double)U[sel[m - 1]][k], the sum
// formed in fp64 per feature (the host loop's `W + X[i].double()`); a sel entry outside [0, n_cand) scores as W.
// One block per (LC_ROWS rows, LC_MODELS models): the block's models are staged in LDS zero-padded to LC_DMAX
// features, every lane keeps one row in registers and takes a sequential fp64 FMA dot per model (the padding
// adds exact zeros); a wave ballot per model gives that wave's misses of either set, kept in lane j for the
// block's model j, then one atomic per (wave, model, set).  The work is ~9000 x 25 x 37 at the RONI shape --
// latency, not throughput: 128-row blocks put that shape on 71 x 3 = 213 blocks, one wave of blocks over the CUs.
// ahead: the evaluation's priority class (k_eval_error_t); RONI runs at the default like k_roni_counts.
// =====================================================================================
#define LC_ROWS 128
#define LC_MODELS 16
#define LC_DMAX 32
extern "C" __global__ void __launch_bounds__(LC_ROWS) k_logit_counts(const double* X, const double* y, int N, int D,
                                                                     int split, const double* W, const float* U,
                                                                     int n_cand, const int* sel, int M, int ahead,
                                                                     unsigned int* counts) {
  if (ahead) BSC_SET_PRIO(BSC_PRIO_AHEAD);
  __shared__ double wm[LC_MODELS][LC_DMAX];
  const int lane = threadIdx.x & 63;
  const int m0 = blockIdx.y * LC_MODELS, nm = min(LC_MODELS, M - m0);
  const long long row = (long long)blockIdx.x * LC_ROWS + threadIdx.x;
  const bool valid = row < N;
  const size_t rl = (size_t)min(row, (long long)N - 1);   // lanes past N load the last row and are not counted
  const double* xr = X + rl * D;
  double x[LC_DMAX];
#pragma unroll
  for (int k = 0; k < LC_DMAX; ++k) x[k] = k < D ? xr[k] : 0.0;
  const double yr = y[rl];
  // the models: thread t forms feature t % LC_DMAX of models t / LC_DMAX + 4 i (every candidate index first, then
  // every update: two dependent global latencies for the block, under the row loads)
  constexpr int kPer = LC_MODELS * LC_DMAX / LC_ROWS, kStep = LC_ROWS / LC_DMAX;
  static_assert(LC_ROWS % LC_DMAX == 0 && kPer * kStep == LC_MODELS && LC_MODELS <= 64, "staging covers wm once");
  const int wk = threadIdx.x % LC_DMAX, wj = threadIdx.x / LC_DMAX;
  const bool kin = wk < D;
  const double wbase = kin ? W[wk] : 0.0;
  int c[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int j = wj + i * kStep, m = m0 + j;
    c[i] = (kin && j < nm && m > 0) ? sel[m - 1] : -1;
  }
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int j = wj + i * kStep;
    double w = j < nm ? wbase : 0.0;
    if (c[i] >= 0 && c[i] < n_cand) w += (double)U[(size_t)c[i] * D + wk];
    wm[j][wk] = w;
  }
  const unsigned long long set0 = __ballot(valid && row < split), set1 = __ballot(valid && row >= split);
  __syncthreads();
  unsigned int c0 = 0, c1 = 0;
  for (int j = 0; j < nm; ++j) {
    double z = 0.0;
#pragma unroll
    for (int k = 0; k < LC_DMAX; ++k) z = __builtin_fma(x[k], wm[j][k], z);
    const double s = (double)((z > 0.0) - (z < 0.0));
    const unsigned long long miss = __ballot(!(s == yr) || z != z);
    if (lane == j) {
      c0 = (unsigned int)__popcll(miss & set0);
      c1 = (unsigned int)__popcll(miss & set1);
    }
  }
  if (lane < nm) {
    unsigned int* out = counts + (size_t)(m0 + lane) * 2;
    if (c0) atomicAdd(out, c0);
    if (c1) atomicAdd(out + 1, c1);
  }
}

// =====================================================================================
// K12: exact recovery of the aggregated chunk polynomials from miner shares.
// ys: int64 [nchunks][npts], xs: int [npts] distinct; deg+1 <= npts.  Newton divided differences
// in 128-bit on the deg+1 nodes of smallest |x|, verified against every share.  Writes the
// dequantised aggregate into W_new = W + coeff / 10^prec  (fp64, the reference's mat.Dense.Add).
// status[k] = 1 exact, 0 inconsistent shares, equal x-points or a coefficient outside int64 -- the cases in
// which the host's recover_exact returns false (caller falls back to least squares).
// =====================================================================================
namespace {
__device__ __forceinline__ bool div_small(__int128 a, long long d, __int128* q) {
  // exact division of a signed 128-bit value by a small non-zero divisor (|d| < 2^31)
  const bool neg = (a < 0) != (d < 0);
  unsigned __int128 m = a < 0 ? (unsigned __int128)(-a) : (unsigned __int128)a;
  const unsigned long long dd = d < 0 ? (unsigned long long)(-d) : (unsigned long long)d;
  const unsigned long long hi = (unsigned long long)(m >> 64), lo = (unsigned long long)m;
  const unsigned long long qh = hi / dd;
  unsigned long long r = hi % dd;
  unsigned long long t = (r << 32) | (lo >> 32);
  const unsigned long long q1 = t / dd;
  r = t % dd;
  t = (r << 32) | (lo & 0xFFFFFFFFull);
  const unsigned long long q0 = t / dd;
  r = t % dd;
  if (r != 0) return false;
  unsigned __int128 qq = ((unsigned __int128)qh << 64) | ((unsigned __int128)q1 << 32) | q0;
  *q = neg ? -(__int128)qq : (__int128)qq;
  return true;
}
}  // namespace

extern "C" __global__ void k_recover(const long long* ys, int nchunks, int npts, const int* xs, int poly, int d,
                                     const double* W, double qscale, double* W_new, long long* coeffs,
                                     int* status) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nchunks) return;
  const int n = poly;  // degree poly-1
  // node choice: smallest |x| first (stable)
  int order[32];
  for (int i = 0; i < npts; ++i) order[i] = i;
  for (int a = 1; a < npts; ++a) {
    const int v = order[a];
    const int av = xs[v] < 0 ? -xs[v] : xs[v];
    int b = a - 1;
    while (b >= 0) {
      const int ob = xs[order[b]] < 0 ? -xs[order[b]] : xs[order[b]];
      if (ob > av || (ob == av && xs[order[b]] > xs[v])) {
        order[b + 1] = order[b];
        --b;
      } else {
        break;
      }
    }
    order[b + 1] = v;
  }
  __int128 nx[16], dd[16], c[16];
  bool ok = npts >= n;
  for (int i = 0; i < n && ok; ++i) {
    nx[i] = xs[order[i]];
    dd[i] = ys[(size_t)k * npts + order[i]];
  }
  for (int lvl = 1; lvl < n && ok; ++lvl)
    for (int i = n - 1; i >= lvl && ok; --i) {
      __int128 q = 0;
      const long long dx = (long long)(nx[i] - nx[i - lvl]);
      // two equal x-points: no polynomial through them (the host's recover_exact returns false)
      ok = dx != 0 && div_small(dd[i] - dd[i - 1], dx, &q);
      dd[i] = q;
    }
  if (ok) {
    for (int i = 0; i < n; ++i) c[i] = 0;
    c[0] = dd[n - 1];
    int cur = 0;
    for (int kk = n - 2; kk >= 0; --kk) {
      for (int j = cur + 1; j >= 1; --j) c[j] = c[j - 1] - nx[kk] * c[j];
      c[0] = -nx[kk] * c[0] + dd[kk];
      ++cur;
    }
    // a coefficient outside int64 is no recovery (recover_exact returns false): the cast below would wrap it
    for (int j = 0; j < n; ++j) ok = ok && c[j] >= (__int128)INT64_MIN && c[j] <= (__int128)INT64_MAX;
    for (int pt = 0; pt < npts && ok; ++pt) {
      __int128 acc = 0;
      for (int j = n - 1; j >= 0; --j) acc = acc * xs[pt] + c[j];
      ok = acc == (__int128)ys[(size_t)k * npts + pt];
    }
  }
  status[k] = ok ? 1 : 0;
  const int prev = k * poly;
  for (int j = 0; j < n; ++j) {
    const long long v = ok ? (long long)c[j] : 0;
    coeffs[(size_t)k * n + j] = v;
    const int idx = prev + j;
    if (idx < d) W_new[idx] = W[idx] + (double)v / qscale;
  }
}

// =====================================================================================
// K12, fused form: share-value sums + exact recovery with precomputed integer weights.
// For a fixed x-point layout (the contributing miners' parts) the inverse Vandermonde on the `poly`
// basis nodes is A / Dn with integer A (host-computed exactly, |A| < 2^40, Dn = 2^s * Dodd), so
// c_j = (sum_i A[j][i] y_{basis_i}) / Dn -- an int128 mat-vec and one exact division, done as a
// shift plus a multiplication by Dodd^-1 mod 2^128 (no 128-bit divisions).  Every share is then
// re-checked by Horner in int128 (status 0 -> the host's least squares, like the old kernel).
// The miners' sums are fused in: agg[k][p] = sum over rows r with mask[r] of ys[r][k][ycols[p]]
// (nrows = 1 and mask = null when ys already holds totals).  One block: 8 chunks.
// =====================================================================================
namespace {
constexpr int RW_CPB = 8;     // chunks per block
constexpr int RW_MAXP = 32;   // points per chunk
constexpr int RW_MAXC = 16;   // coefficients per chunk
}  // namespace

extern "C" __global__ void __launch_bounds__(256) k_recover_w(
    const long long* ys, int nrows, long long rstride, int nch, int T, const int* mask, const int* ycols, const int* xs, int npts,
    const long long* A, const int* basis, int poly, int shift, unsigned long long inv_lo, unsigned long long inv_hi,
    int d, const double* W, double qscale, double* W_new, long long* coeffs, int* status, long long* agg_out,
    double* h_W, int* h_status, long long* h_clock) {
  BSC_SET_PRIO(BSC_PRIO_CRITICAL);
  // several ranks (h_clock): each rank's row carries its clock right after its share sums -- block 0 mirrors
  // them to the host with the model (no strided read-back copy behind the kernel)
  if (h_clock != nullptr && blockIdx.x == 0 && threadIdx.x < nrows)
    h_clock[threadIdx.x] = ys[(size_t)threadIdx.x * rstride + (size_t)nch * T];
  __shared__ long long agg[RW_CPB][RW_MAXP];
  __shared__ __int128 cf[RW_CPB][RW_MAXC];
  __shared__ int ok[RW_CPB];
  const int t = threadIdx.x;
  const int k0 = blockIdx.x * RW_CPB;
  if (t < RW_CPB) ok[t] = 1;
  // 1. the miners' share sums for this block's chunks
  for (int e = t; e < RW_CPB * npts; e += 256) {
    const int c = e / npts, p = e % npts, k = k0 + c;
    if (k >= nch) continue;
    long long s = 0;
    const int col = ycols[p];
    for (int r = 0; r < nrows; ++r)
      if (mask == nullptr || mask[r]) s += ys[(size_t)r * rstride + (size_t)k * T + col];
    agg[c][p] = s;
    agg_out[(size_t)k * npts + p] = s;
  }
  __syncthreads();
  // 2. coefficients: int128 mat-vec, exact division by Dn = 2^shift * Dodd
  const unsigned __int128 inv = ((unsigned __int128)inv_hi << 64) | inv_lo;
  for (int e = t; e < RW_CPB * poly; e += 256) {
    const int c = e / poly, j = e % poly;
    if (k0 + c >= nch) continue;
    __int128 n = 0;
    for (int i = 0; i < poly; ++i) n += (__int128)A[j * poly + i] * (__int128)agg[c][basis[i]];
    bool exact = (shift == 0) || ((n & ((((__int128)1) << shift) - 1)) == 0);
    const __int128 q = (__int128)((unsigned __int128)(n >> shift) * inv);
    // a true coefficient is tiny next to 2^100; an inexact division lands anywhere in 2^128
    const __int128 lim = ((__int128)1) << 100;
    exact = exact && q < lim && q > -lim;
    // and one outside int64 is no recovery (the host's recover_exact returns false): the cast in step 4 would wrap it
    exact = exact && q >= (__int128)INT64_MIN && q <= (__int128)INT64_MAX;
    cf[c][j] = q;
    if (!exact) atomicAnd(&ok[c], 0);
  }
  __syncthreads();
  // 3. every share must lie on the recovered polynomial (Horner, int128)
  for (int e = t; e < RW_CPB * npts; e += 256) {
    const int c = e / npts, p = e % npts;
    if (k0 + c >= nch) continue;
    __int128 acc = 0;
    const __int128 x = xs[p];
    for (int j = poly - 1; j >= 0; --j) acc = acc * x + cf[c][j];
    if (acc != (__int128)agg[c][p]) atomicAnd(&ok[c], 0);
  }
  __syncthreads();
  // 4. outputs: coefficients, dequantised model update
  for (int e = t; e < RW_CPB * poly; e += 256) {
    const int c = e / poly, j = e % poly, k = k0 + c;
    if (k >= nch) continue;
    const bool good = ok[c] != 0;
    const long long v = good ? (long long)cf[c][j] : 0;
    coeffs[(size_t)k * poly + j] = v;
    if (j == 0) {
      status[k] = good ? 1 : 0;
      if (h_status != nullptr) h_status[k] = good ? 1 : 0;
    }
    const int idx = k * poly + j;
    if (idx < d) {
      const double w = W[idx] + (double)v / qscale;
      W_new[idx] = w;
      if (h_W != nullptr) h_W[idx] = w;   // pinned host mirror: the host reads it after the kernel's event
    }
  }
  // (no system-scope fence: the host reads the mirrors only after the kernel's completion event, whose
  // end-of-kernel release makes them visible; a fence per block was an L2 write-back per block on the chain)
}

// =====================================================================================
// Plain aggregation (non-secure-agg / FedSys): W_new = W + sum_r delta64[rows[r]] in fp64,
// in row order (mat.Dense.Add sequence).
// =====================================================================================
extern "C" __global__ void k_add_rows(const float* delta, int D, const int* rows, int nrows, const double* W,
                                      double* W_new) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D) return;
  double acc = W[i];
  for (int r = 0; r < nrows; ++r) acc += (double)delta[(size_t)rows[r] * D + i];
  W_new[i] = acc;
}

// ---------------------------------------------------------------- C ABI launchers
static inline int nblk(long long n, int bs) { return (int)((n + bs - 1) / bs); }

// =====================================================================================
// K11 (several ranks): a rank's partial share-value sums of its kept rows, exact in int64:
// out[c] = sum over selected rows r of ys[r][c], c < C (C = nchunks * TOTAL_SHARES).  Rows come from an
// index list, a device-side selection mask (the committee's block mask) or all rows.  One thread per
// column; consecutive threads read consecutive columns of a row (coalesced), rows in order (exact and
// order-independent anyway: integer adds).  The sums go straight into the aggregation's all_gather.
// =====================================================================================
extern "C" __global__ void __launch_bounds__(256) k_sum_rows_i64(const long long* __restrict__ ys, int R, long long C,
                                                                const int* __restrict__ rows, int nsel,
                                                                const int* __restrict__ mask,
                                                                long long* __restrict__ out) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  long long s = 0;
  for (int i = 0; i < nsel; ++i) {
    const int r = rows != nullptr ? rows[i] : i;
    if (r < 0 || r >= R) continue;
    if (mask != nullptr && !mask[r]) continue;
    s += ys[(size_t)r * C + c];
  }
  out[c] = s;
}

extern "C" int bsc_sum_rows_i64(const long long* ys, int R, long long C, const int* rows, int nsel, const int* mask,
                                long long* out, void* stream) {
  if (C <= 0) return 0;
  if (rows == nullptr) nsel = R;
  hipLaunchKernelGGL(k_sum_rows_i64, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ys, R, C,
                     rows, nsel, mask, out);
  return (int)hipGetLastError();
}

// the same sums with one more int64 after them: out[C] = tail (the multi-rank send row's clock, kernels/round.hip)
// -- written by the sums' own launch instead of two memset launches behind it on the critical path; R = 0: zeros
extern "C" __global__ void __launch_bounds__(256) k_sum_rows_i64_tail(const long long* __restrict__ ys, int R,
                                                                     long long C, const int* __restrict__ mask,
                                                                     long long* __restrict__ out, long long tail) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > C) return;
  if (c == C) {
    out[C] = tail;
    return;
  }
  long long s = 0;
  for (int r = 0; r < R; ++r)
    if (mask == nullptr || mask[r]) s += ys[(size_t)r * C + c];
  out[c] = s;
}

extern "C" int bsc_sum_rows_i64_tail(const long long* ys, int R, long long C, const int* mask, long long* out,
                                     long long tail, void* stream) {
  if (C < 0 || R < 0 || (R > 0 && ys == nullptr)) return -1;
  hipLaunchKernelGGL(k_sum_rows_i64_tail, dim3((unsigned)((C + 1 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ys, R, C, mask, out, tail);
  return (int)hipGetLastError();
}

extern "C" int bsc_softmax_step(const float* X, const int* y, const long long* off, const int* ntrain,
                                const int* pid, const double* W, int D_IN, int D_OUT, int B, int P, unsigned long long seed,
                                int iteration, float max_norm, double qscale, float* delta, long long* qdelta,
                                float* loss, int lo, int* ones, int nones, void* stream) {
  if (D_IN <= 0 || D_OUT > 16 || B > 16) return -1;
  if (P <= 0) return 0;
  hipLaunchKernelGGL(k_softmax_step, dim3(P), dim3(SM_THREADS), 0, (hipStream_t)stream, X, y, off, ntrain, pid, W, D_IN,
                     D_OUT, B, P, seed, iteration, max_norm, qscale, delta, qdelta, loss, lo, ones, nones);
  return (int)hipGetLastError();
}

// the margin form: bsc_softmax_step's arguments, limits and geometry
extern "C" int bsc_margin_step(const float* X, const int* y, const long long* off, const int* ntrain,
                               const int* pid, const double* W, int D_IN, int D_OUT, int B, int P, unsigned long long seed,
                               int iteration, float max_norm, double qscale, float* delta, long long* qdelta,
                               float* loss, int lo, int* ones, int nones, void* stream) {
  if (D_IN <= 0 || D_OUT > 16 || B > 16) return -1;
  if (P <= 0) return 0;
  hipLaunchKernelGGL(k_margin_step, dim3(P), dim3(SM_THREADS), 0, (hipStream_t)stream, X, y, off, ntrain, pid, W, D_IN,
                     D_OUT, B, P, seed, iteration, max_norm, qscale, delta, qdelta, loss, lo, ones, nones);
  return (int)hipGetLastError();
}

// K1m: bsc_softmax_step's arguments and limits with H hidden units in front of D_OUT (a multiple of 16 up to 64)
// and W in the MLP's layout; no speculative row flags (the ledger does not run this model)
extern "C" int bsc_mlp_step(const float* X, const int* y, const long long* off, const int* ntrain, const int* pid,
                            const double* W, int D_IN, int H, int D_OUT, int B, int P, unsigned long long seed,
                            int iteration, float max_norm, double qscale, float* delta, long long* qdelta, float* loss,
                            int lo, void* stream) {
  if (D_IN <= 0 || D_OUT < 1 || D_OUT > 16 || B > 16 || H < 16 || H > 64 || H % 16 != 0) return -1;
  if (P <= 0) return 0;
#define BSC_MLP_STEP(NCT)                                                                                            \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mlp_step<NCT>), dim3(P), dim3(256), 0, (hipStream_t)stream, X, y, off, ntrain, \
                     pid, W, D_IN, D_OUT, B, P, seed, iteration, max_norm, qscale, delta, qdelta, loss, lo)
  switch (H / 16) {
    case 1: BSC_MLP_STEP(1); break;
    case 2: BSC_MLP_STEP(2); break;
    case 3: BSC_MLP_STEP(3); break;
    default: BSC_MLP_STEP(4); break;
  }
#undef BSC_MLP_STEP
  return (int)hipGetLastError();
}

// K1c: bsc_softmax_step's arguments and limits with the image side S (1..28, D_IN = S * S) in D_IN's place, W in the
// CNN's layout and the step rate lr > 0 behind qscale; no speculative row flags (the ledger does not run this model)
extern "C" int bsc_cnn_step(const float* X, const int* y, const long long* off, const int* ntrain, const int* pid,
                            const double* W, int S, int D_OUT, int B, int P, unsigned long long seed, int iteration,
                            float max_norm, double qscale, float lr, float* delta, long long* qdelta, float* loss,
                            int lo, void* stream) {
  if (S < 1 || S > CNN_SMAX || D_OUT < 1 || D_OUT > 16 || B > 16 || !(lr > 0.f)) return -1;
  if (P <= 0) return 0;
  // K1c's images and stage buffers pass the default 64 KiB of LDS: opt in once
  static const hipError_t optin =
      hipFuncSetAttribute((const void*)k_cnn_step, hipFuncAttributeMaxDynamicSharedMemorySize, CNN_DYN_LDS);
  if (optin != hipSuccess) return (int)optin;
  hipLaunchKernelGGL(k_cnn_step, dim3(P), dim3(256), CNN_DYN_LDS, (hipStream_t)stream, X, y, off, ntrain, pid, W, S,
                     D_OUT, B, P, seed, iteration, max_norm, qscale, lr, delta, qdelta, loss, lo);
  return (int)hipGetLastError();
}

namespace {
template <class Loss>
int local_steps_launch(hipStream_t s, int nparam, const float* X, const int* y, const long long* off, const int* ntrain,
                       const int* pid, const double* W, int D_IN, int D_OUT, int B, int P, unsigned long long seed,
                       int iteration, float max_norm, double qscale, int E, float lr, float* delta, long long* qdelta,
                       float* loss, int lo, int* ones, int nones) {
  if (nparam <= LS_LDS_A)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_local_steps<Loss, true>), dim3(P), dim3(SM_THREADS),
                       (size_t)nparam * sizeof(float), s, X, y, off, ntrain, pid, W, D_IN, D_OUT, B, P, seed, iteration,
                       max_norm, qscale, E, lr, delta, qdelta, loss, lo, ones, nones);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_local_steps<Loss, false>), dim3(P), dim3(SM_THREADS), 0, s, X, y, off, ntrain,
                       pid, W, D_IN, D_OUT, B, P, seed, iteration, max_norm, qscale, E, lr, delta, qdelta, loss, lo,
                       ones, nones);
  return (int)hipGetLastError();
}
}  // namespace

// K1e: E local steps at rate lr under loss 0 (cross-entropy) or 1 (margin); K1's arguments and limits otherwise.
// a lives in LDS up to LS_LDS_A parameters, in the delta rows beyond.
extern "C" int bsc_local_steps(int loss, const float* X, const int* y, const long long* off, const int* ntrain,
                               const int* pid, const double* W, int D_IN, int D_OUT, int B, int P,
                               unsigned long long seed, int iteration, float max_norm, double qscale, int E, float lr,
                               float* delta, long long* qdelta, float* loss_out, int lo, int* ones, int nones,
                               void* stream) {
  if (D_IN <= 0 || D_OUT > 16 || B > 16 || E < 1 || E > LS_MAX_E || !(lr > 0.f) || loss < 0 || loss > 1) return -1;
  if (P <= 0) return 0;
  const int nparam = D_OUT * D_IN + D_OUT;
  return loss == 1 ? local_steps_launch<MarginLoss>((hipStream_t)stream, nparam, X, y, off, ntrain, pid, W, D_IN, D_OUT,
                                                    B, P, seed, iteration, max_norm, qscale, E, lr, delta, qdelta,
                                                    loss_out, lo, ones, nones)
                   : local_steps_launch<CrossEntropyLoss>((hipStream_t)stream, nparam, X, y, off, ntrain, pid, W, D_IN,
                                                          D_OUT, B, P, seed, iteration, max_norm, qscale, E, lr, delta,
                                                          qdelta, loss_out, lo, ones, nones);
}

namespace {
template <class Loss, bool MOM>
int momentum_steps_launch(hipStream_t s, int nparam, const float* X, const int* y, const long long* off,
                          const int* ntrain, const int* pid, const double* W, int D_IN, int D_OUT, int B, int P,
                          unsigned long long seed, int iteration, float max_norm, double qscale, int E, float lr,
                          float mom, float decay, float prox, float* delta, long long* qdelta, float* loss,
                          float* vwork, int lo, int* ones, int nones) {
  if (nparam <= LS_LDS_A) {
    if (MOM) {
      // a and v beside the static 31016 B pass the default 64 KiB (K1m's header): opt in once per instance
      static const hipError_t optin =
          hipFuncSetAttribute((const void*)k_momentum_steps<Loss, true, MOM>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 2 * LS_LDS_A * (int)sizeof(float));
      if (optin != hipSuccess) return (int)optin;
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_momentum_steps<Loss, true, MOM>), dim3(P), dim3(SM_THREADS),
                       (size_t)(MOM ? 2 : 1) * nparam * sizeof(float), s, X, y, off, ntrain, pid, W, D_IN, D_OUT, B, P,
                       seed, iteration, max_norm, qscale, E, lr, mom, decay, prox, delta, qdelta, loss, vwork, lo, ones,
                       nones);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_momentum_steps<Loss, false, MOM>), dim3(P), dim3(SM_THREADS), 0, s, X, y, off,
                       ntrain, pid, W, D_IN, D_OUT, B, P, seed, iteration, max_norm, qscale, E, lr, mom, decay, prox,
                       delta, qdelta, loss, vwork, lo, ones, nones);
  }
  return (int)hipGetLastError();
}
}  // namespace

// K1m: K1e's E local steps with momentum mom in [0, 1), weight decay >= 0 and proximal weight prox >= 0 (all finite).
// vwork: fp32 [P, nparam] velocity workspace, needed when mom > 0 and nparam > LS_LDS_A (else nullable, untouched); it
// needs no clearing.  The other arguments and limits are K1e's.
extern "C" int bsc_momentum_steps(int loss, const float* X, const int* y, const long long* off, const int* ntrain,
                                  const int* pid, const double* W, int D_IN, int D_OUT, int B, int P,
                                  unsigned long long seed, int iteration, float max_norm, double qscale, int E, float lr,
                                  float momentum, float decay, float prox, float* delta, long long* qdelta,
                                  float* loss_out, float* vwork, int lo, int* ones, int nones, void* stream) {
  if (D_IN <= 0 || D_OUT > 16 || B > 16 || E < 1 || E > LS_MAX_E || !(lr > 0.f) || loss < 0 || loss > 1) return -1;
  if (!(momentum >= 0.f && momentum < 1.f) || !(decay >= 0.f && decay < INFINITY) || !(prox >= 0.f && prox < INFINITY))
    return -1;
  const int nparam = D_OUT * D_IN + D_OUT;
  const bool m = momentum > 0.f;
  if (m && nparam > LS_LDS_A && vwork == nullptr) return -1;
  if (P <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
#define BSC_MOM_LAUNCH(LOSS, MOMV)                                                                                    \
  momentum_steps_launch<LOSS, MOMV>(s, nparam, X, y, off, ntrain, pid, W, D_IN, D_OUT, B, P, seed, iteration,         \
                                    max_norm, qscale, E, lr, momentum, decay, prox, delta, qdelta, loss_out, vwork,   \
                                    lo, ones, nones)
  if (loss == 1) return m ? BSC_MOM_LAUNCH(MarginLoss, true) : BSC_MOM_LAUNCH(MarginLoss, false);
  return m ? BSC_MOM_LAUNCH(CrossEntropyLoss, true) : BSC_MOM_LAUNCH(CrossEntropyLoss, false);
#undef BSC_MOM_LAUNCH
}

namespace {
template <class Loss>
int dpsgd_steps_launch(hipStream_t s, int nparam, const float* X, const int* y, const long long* off, const int* ntrain,
                       const int* pid, const double* W, int D_IN, int D_OUT, int B, int P, unsigned long long seed,
                       int iteration, double qscale, float clip, float sigma, int E, float lr, float* delta,
                       long long* qdelta, float* loss, int lo, int* ones, int nones) {
  if (nparam <= LS_LDS_A)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dpsgd_steps<Loss, true>), dim3(P), dim3(SM_THREADS),
                       (size_t)nparam * sizeof(float), s, X, y, off, ntrain, pid, W, D_IN, D_OUT, B, P, seed, iteration,
                       qscale, clip, sigma, E, lr, delta, qdelta, loss, lo, ones, nones);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dpsgd_steps<Loss, false>), dim3(P), dim3(SM_THREADS), 0, s, X, y, off, ntrain,
                       pid, W, D_IN, D_OUT, B, P, seed, iteration, qscale, clip, sigma, E, lr, delta, qdelta, loss, lo,
                       ones, nones);
  return (int)hipGetLastError();
}
}  // namespace

// K1p: E DP-SGD steps at rate lr under loss 0 (cross-entropy) or 1 (margin): per-example clip at `clip` (> 0), noise
// multiplier `sigma` (>= 0; 0 draws nothing); K1e's arguments and limits otherwise, and its placement of a.
extern "C" int bsc_dpsgd_steps(int loss, const float* X, const int* y, const long long* off, const int* ntrain,
                               const int* pid, const double* W, int D_IN, int D_OUT, int B, int P,
                               unsigned long long seed, int iteration, double qscale, float clip, float sigma, int E,
                               float lr, float* delta, long long* qdelta, float* loss_out, int lo, int* ones, int nones,
                               void* stream) {
  if (D_IN <= 0 || D_OUT > 16 || B > 16 || E < 1 || E > LS_MAX_E || !(lr > 0.f) || !(clip > 0.f) || !(sigma >= 0.f) ||
      loss < 0 || loss > 1)
    return -1;
  if (P <= 0) return 0;
  const int nparam = D_OUT * D_IN + D_OUT;
  return loss == 1 ? dpsgd_steps_launch<MarginLoss>((hipStream_t)stream, nparam, X, y, off, ntrain, pid, W, D_IN, D_OUT,
                                                    B, P, seed, iteration, qscale, clip, sigma, E, lr, delta, qdelta,
                                                    loss_out, lo, ones, nones)
                   : dpsgd_steps_launch<CrossEntropyLoss>((hipStream_t)stream, nparam, X, y, off, ntrain, pid, W, D_IN,
                                                          D_OUT, B, P, seed, iteration, qscale, clip, sigma, E, lr,
                                                          delta, qdelta, loss_out, lo, ones, nones);
}

namespace {
template <class Loss, bool DP>
int lot_steps_launch(hipStream_t s, int nparam, const float* X, const int* y, const long long* off, const int* ntrain,
                     const int* pid, const double* W, int D_IN, int D_OUT, int L, int P, unsigned long long seed,
                     int iteration, float max_norm, double qscale, float clip, float sigma, int E, float lr,
                     float* delta, long long* qdelta, float* loss, float* gwork, int lo, int* ones, int nones) {
  if (nparam <= LS_LDS_A) {
    // static + dynamic LDS passes the default 64 KiB (K1l's header): opt in once per instance, up to a (and g) at LS_LDS_A
    static const hipError_t optin =
        hipFuncSetAttribute((const void*)k_lot_steps<Loss, true, DP>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (DP ? 1 : 2) * LS_LDS_A * (int)sizeof(float));
    if (optin != hipSuccess) return (int)optin;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lot_steps<Loss, true, DP>), dim3(P), dim3(SM_THREADS),
                       (size_t)(DP ? 1 : 2) * nparam * sizeof(float), s, X, y, off, ntrain, pid, W, D_IN, D_OUT, L, P,
                       seed, iteration, max_norm, qscale, clip, sigma, E, lr, delta, qdelta, loss, gwork, lo, ones,
                       nones);
  } else {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lot_steps<Loss, false, DP>), dim3(P), dim3(SM_THREADS), 0, s, X, y, off,
                       ntrain, pid, W, D_IN, D_OUT, L, P, seed, iteration, max_norm, qscale, clip, sigma, E, lr, delta,
                       qdelta, loss, gwork, lo, ones, nones);
  }
  return (int)hipGetLastError();
}
}  // namespace

// K1l: E local steps on lots of L <= LOT_MAX examples under loss 0 (cross-entropy) or 1 (margin).  clip == 0: K1e's
// rule (the mean gradient clipped at max_norm); clip > 0: K1p's (per-example clip, noise multiplier sigma >= 0, and
// max_norm unused).  gwork: fp32 [P, nparam] step-gradient workspace, needed when clip == 0 and nparam > LS_LDS_A
// (else nullable, untouched).  The other arguments and limits are K1e's.
extern "C" int bsc_lot_steps(int loss, const float* X, const int* y, const long long* off, const int* ntrain,
                             const int* pid, const double* W, int D_IN, int D_OUT, int L, int P,
                             unsigned long long seed, int iteration, float max_norm, double qscale, float clip,
                             float sigma, int E, float lr, float* delta, long long* qdelta, float* loss_out,
                             float* gwork, int lo, int* ones, int nones, void* stream) {
  if (D_IN <= 0 || D_OUT > 16 || L < 1 || L > LOT_MAX || E < 1 || E > LS_MAX_E || !(lr > 0.f) || !(clip >= 0.f) ||
      !(sigma >= 0.f) || (sigma > 0.f && !(clip > 0.f)) || loss < 0 || loss > 1)
    return -1;
  const int nparam = D_OUT * D_IN + D_OUT;
  const bool dp = clip > 0.f;
  if (!dp && nparam > LS_LDS_A && gwork == nullptr) return -1;
  if (P <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
#define BSC_LOT_LAUNCH(LOSS, DPV)                                                                                     \
  lot_steps_launch<LOSS, DPV>(s, nparam, X, y, off, ntrain, pid, W, D_IN, D_OUT, L, P, seed, iteration, max_norm,     \
                              qscale, clip, sigma, E, lr, delta, qdelta, loss_out, gwork, lo, ones, nones)
  if (loss == 1) return dp ? BSC_LOT_LAUNCH(MarginLoss, true) : BSC_LOT_LAUNCH(MarginLoss, false);
  return dp ? BSC_LOT_LAUNCH(CrossEntropyLoss, true) : BSC_LOT_LAUNCH(CrossEntropyLoss, false);
#undef BSC_LOT_LAUNCH
}

// K1t on delta fp32 [P, D] / qdelta int64 [P, D] in place; kept (nullable) int32 [P].  k == D keeps everything:
// nothing is launched (and kept is not written).
extern "C" int bsc_topk_rows(float* delta, long long* qdelta, int P, int D, int k, int* kept, void* stream) {
  if (D <= 0 || k < 1 || k > D) return -1;
  if (P <= 0 || k == D) return 0;
  if (D <= TK_LDS_KEYS)
    hipLaunchKernelGGL(k_topk_rows, dim3(P), dim3(TK_THREADS), (size_t)D * sizeof(uint32_t), (hipStream_t)stream,
                       delta, qdelta, D, k, kept);
  else
    hipLaunchKernelGGL(k_topk_rows_stream, dim3(P), dim3(TK_THREADS), 0, (hipStream_t)stream, delta, qdelta, D, k,
                       kept);
  return (int)hipGetLastError();
}

extern "C" int bsc_logreg_step(const double* X, const double* y, const long long* off, const int* nrows,
                               const int* pid, const double* W, int D, int B, int P, unsigned long long seed, const int* calls,
                               double alpha, double lammy, const double* sigma, double qscale, float* delta,
                               long long* qdelta, void* stream) {
  if (B > 64) return -1;
  if (P <= 0) return 0;
  hipLaunchKernelGGL(k_logreg_step, dim3(P), dim3(64), 0, (hipStream_t)stream, X, y, off, nrows, pid, W, D, B, P, seed,
                     calls, alpha, lammy, sigma, qscale, delta, qdelta);
  return (int)hipGetLastError();
}

extern "C" int bsc_dp_noise(const float* delta, int P, int D, const int* noisers, int nn, const float* scale,
                            unsigned long long seed, int iter_mod, float* noised, void* stream) {
  const long long n = (long long)P * D;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_dp_noise, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, delta, P, D, noisers, nn,
                     scale, seed, iter_mod, noised);
  return (int)hipGetLastError();
}

// Single-verifier Multi-Krum (K5a-c): X [n, D] fp32; part [ceil(D/ksplit), npad, npad] f64 scratch with
// npad = 16 * ceil(n/16); dist [n, n], scores [n] f64; accept [n] int32.  n <= 0: no-op, returns 0;
// n > 128, D <= 0 or ksplit <= 0: returns -1.
extern "C" int bsc_krum(const float* X, int n, int D, int ksplit, double* part, double* dist, double* scores,
                        int* accept, int groupsize, int n_accept, void* stream) {
  if (n <= 0) return 0;
  if (n > 128 || D <= 0 || ksplit <= 0) return -1;   // nothing is launched or written
  const int tiles = (n + 15) / 16;
  const int nsplit = (int)(((long long)D + ksplit - 1) / ksplit);
  hipLaunchKernelGGL(k_gram_f64, dim3(tiles, tiles, nsplit), dim3(64), 0, (hipStream_t)stream, X, n, D, ksplit,
                     part);
  hipLaunchKernelGGL(k_krum_scores, dim3(n), dim3(64), 0, (hipStream_t)stream, part, nsplit, n, tiles * 16,
                     groupsize, dist, scores);
  hipLaunchKernelGGL(k_krum_accept, dim3(1), dim3(128), 0, (hipStream_t)stream, scores, n, n_accept, accept);
  return (int)hipGetLastError();
}

// Committee Multi-Krum: X [U, D] fp32; inbox [V, n] rows of X; lead_rank [U] (-1: not submitted).
// part: [nsplit, npairs, 256] f64 scratch (npairs = T(T+1)/2, T = ceil(U/16), nsplit = ceil(D/kchunk));
// scores [V, n] f64; acc [V, n] int32; node [U] int32.
// Limits: U <= 8192 candidate rows, inbox n <= 4096, V <= 64 verifiers; ws: int32 [U] workspace
// (used when n > 256 or U > 1024).
extern "C" int bsc_krum_committee(const float* X, int U, int D, int kchunk, const int* inbox, int V, int n,
                                  int groupsize, int n_accept, int need, const int* lead_rank, int cap, double* part,
                                  double* gram, unsigned int* count, double* scores, int* acc, int* node, int* ws,
                                  void* stream) {
  if (U <= 0 || V <= 0 || n <= 0) return 0;
  if (U > 8192 || n > 4096 || V > 64 || n > U || kchunk <= 0) return -1;
  const int T = (U + 15) / 16;
  const int npairs = T * (T + 1) / 2;
  const int nsplit = (D + kchunk - 1) / kchunk;
  hipStream_t s = (hipStream_t)stream;
  // count: npairs zeroed counters (re-armed by the kernel itself)
  hipLaunchKernelGGL(k_gram_pairs, dim3(npairs, nsplit), dim3(256), 0, s, X, U, D, kchunk, T, part, gram, count,
                     (const float*)nullptr, U, 0ll, 0, (const double*)nullptr, 0);
  hipLaunchKernelGGL(k_gram_reduce, dim3(npairs), dim3(256), 0, s, part, gram, npairs, nsplit, 0, T, 0, 0);
  if (n <= 256) {
    hipLaunchKernelGGL(k_krum_rows, dim3(n, V), dim3(256), 0, s, gram, T, inbox, n, groupsize, scores);
  } else {
    const int np2 = pow2_at_least(n);
    hipLaunchKernelGGL(k_krum_rows_big<PlainDot>, dim3(n, V), dim3(1024), (size_t)np2 * sizeof(double), s,
                       PlainDot{gram, T}, inbox, n, np2, groupsize, scores);
  }
  if (krum_vote_any(s, scores, inbox, V, n, n_accept, U, need, lead_rank, cap, acc, node, ws) != 0) return -1;
  return (int)hipGetLastError();
}
// Tile pairs [p0, p1) of the stacked Gram only (p1 <= 0: all of them): several ranks split one Gram's tiles
// and exchange the reduced tiles (engine: the verification all_gather).  part: [nsplit, p1 - p0, 256].
// nn (nullable): this iteration's dense [U2, U2] Gram of the noise rows (setup, bsc_gram_noise_table); the tile
// pairs of noise rows only are copied from it instead of computed.
extern "C" int bsc_gram_stacked_range(const float* X, int U1, const float* X2, int U2, long long stride2, int D,
                                      int kchunk, int p0, int p1, double* part, double* gram, unsigned int* count,
                                      const double* nn, void* stream) {
  const int U = U1 + U2;
  if (U <= 0) return 0;
  if (U > 8192 || kchunk <= 0) return -1;
  const int T = (U + 15) / 16;
  const int npairs = T * (T + 1) / 2;
  if (p1 <= 0 || p1 > npairs) p1 = npairs;
  if (p0 < 0 || p0 > p1) return -1;
  if (p0 == p1) return 0;
  const int nsplit = (D + kchunk - 1) / kchunk;
  hipLaunchKernelGGL(k_gram_pairs, dim3(p1 - p0, nsplit), dim3(256), 0, (hipStream_t)stream, X, U, D, kchunk, T, part,
                     gram, count, X2, U1, stride2, p0, nn, (U1 + 15) / 16);
  hipLaunchKernelGGL(k_gram_reduce, dim3(p1 - p0), dim3(256), 0, (hipStream_t)stream, part, gram, p1 - p0, nsplit, p0,
                     T, (U1 + 15) / 16, nn != nullptr ? 1 : 0);
  return (int)hipGetLastError();
}
namespace {
// the noise-aware committee Krum on a finished stacked Gram: rows kernel, then the vote.  nz / sc [U1][nn] are
// device arrays, or (host_tabs) host arrays that travel in the rows kernel's argument block -- which holds
// U1 * nn <= NOISE_ARG_MAX entries and exists for n <= 256 only; else -2
int krum_committee_noise_any(const double* gram, int U1, int U, const int* nz, const float* sc, bool host_tabs,
                             int nn, const int* inbox, int V, int n, int groupsize, int n_accept, int need,
                             const int* lead_rank, int cap, double* scores, int* acc, int* node, int* ws, int* h_out,
                             const int* amap, int nspec, int* alive, void* stream) {
  if (U1 <= 0 || V <= 0 || n <= 0) return 0;
  if (U > 8192 || U1 > 8192 || n > 4096 || V > 64 || n > U1 || nn <= 0 || nn > 16) return -1;
  if (host_tabs && ((long long)U1 * nn > NOISE_ARG_MAX || n > 256)) return -2;
  const int T = (U + 15) / 16;
  hipStream_t s = (hipStream_t)stream;
  if (host_tabs) {
    NoiseArg q;
    for (int i = 0; i < U1 * nn; ++i) {
      q.nz[i] = nz[i];
      q.sc[i] = sc[i];
    }
    hipLaunchKernelGGL(k_krum_rows_noise_ka, dim3(n, V), dim3(256), 0, s, gram, T, U1, q, nn, inbox, n, groupsize,
                       scores);
  } else if (n <= 256) {
    hipLaunchKernelGGL(k_krum_rows_noise, dim3(n, V), dim3(256), 0, s, gram, T, U1, nz, sc, nn, inbox, n, groupsize,
                       scores);
  } else {
    const int np2 = pow2_at_least(n);
    hipLaunchKernelGGL(k_krum_rows_big<NoiseDot<NoisePtr>>, dim3(n, V), dim3(1024), (size_t)np2 * sizeof(double), s,
                       NoiseDot<NoisePtr>{gram, T, U1, {nz, sc}, nn}, inbox, n, np2, groupsize, scores);
  }
  if (krum_vote_any(s, scores, inbox, V, n, n_accept, U1, need, lead_rank, cap, acc, node, ws, h_out, amap, nspec,
                    alive) != 0)
    return -1;
  return (int)hipGetLastError();
}
}  // namespace
// h_out (nullable): [V * n + U1] pinned host mirror of (acc, node), written by the vote itself (acc and node
// must be contiguous there too); amap / nspec / alive (nullable): the speculative MSM's row flags set in the
// same kernel
extern "C" int bsc_krum_committee_noise2(const double* gram, int U1, int U, const int* nz, const float* sc, int nn,
                                         const int* inbox, int V, int n, int groupsize, int n_accept, int need,
                                         const int* lead_rank, int cap, double* scores, int* acc, int* node, int* ws,
                                         int* h_out, const int* amap, int nspec, int* alive, void* stream) {
  return krum_committee_noise_any(gram, U1, U, nz, sc, false, nn, inbox, V, n, groupsize, n_accept, need, lead_rank,
                                  cap, scores, acc, node, ws, h_out, amap, nspec, alive, stream);
}
// the same with the noisers' ids / weights read from HOST memory (nz_host / sc_host [U1][nn]); -2: the caller
// uploads them and uses the above
extern "C" int bsc_krum_committee_noise_ka(const double* gram, int U1, int U, const int* nz_host, const float* sc_host,
                                           int nn, const int* inbox, int V, int n, int groupsize, int n_accept,
                                           int need, const int* lead_rank, int cap, double* scores, int* acc, int* node,
                                           int* ws, int* h_out, const int* amap, int nspec, int* alive, void* stream) {
  return krum_committee_noise_any(gram, U1, U, nz_host, sc_host, true, nn, inbox, V, n, groupsize, n_accept, need,
                                  lead_rank, cap, scores, acc, node, ws, h_out, amap, nspec, alive, stream);
}
// the evaluation with its accumulator reset and its read-back into pinned memory in one call (the engine
// queues it every round; three Python-level stream operations cost more host time than the kernel)
extern "C" int bsc_eval_error_rb(const float* X, const int* y, int N, int D_IN, int D_OUT, const double* W,
                                 int transform, int split, unsigned int* err, unsigned int* err_host, void* stream) {
  if (hipMemsetAsync(err, 0, 2 * sizeof(unsigned int), (hipStream_t)stream) != hipSuccess) return -1;
  if (D_OUT > 16 || D_IN <= 0) return -1;
  if (N > 0) {
    hipLaunchKernelGGL(k_eval_error, dim3((N + 15) / 16), dim3(256), 0, (hipStream_t)stream, X, y, N, D_IN, D_OUT, W,
                       transform, split, err);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
  }
  return (int)hipMemcpyAsync(err_host, err, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, (hipStream_t)stream);
}

extern "C" int bsc_eval_error_t_rb(const float* Xt, const int* y, int N, int KG, int D_IN, int D_OUT, const double* W,
                                   int split, unsigned int* err, unsigned int* err_host, void* stream) {
  if (D_OUT > 16 || D_IN <= 0 || KG * 4 < D_IN) return -1;
  if (N <= 0) {
    if (hipMemsetAsync(err, 0, 3 * sizeof(unsigned int), (hipStream_t)stream) != hipSuccess) return -1;
    return (int)hipMemcpyAsync(err_host, err, 2 * sizeof(unsigned int), hipMemcpyDeviceToHost, (hipStream_t)stream);
  }
  // err: 3 zeroed counters; k_eval_finish writes err_host and re-zeroes them
  hipLaunchKernelGGL(k_eval_error_t, dim3((N + 15) / 16), dim3(256), 0, (hipStream_t)stream, Xt, y, N, KG, D_IN, D_OUT,
                     W, split, err, err_host);
  hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, err, err_host);
  return (int)hipGetLastError();
}

// K2m with bsc_eval_error_t_rb's hand-off: err holds 3 zeroed counters, k_eval_finish writes err_host and re-zeroes them
extern "C" int bsc_mlp_eval_rb(const float* X, const int* y, int N, int D_IN, int H, int D_OUT, const double* W,
                               int transform, int split, unsigned int* err, unsigned int* err_host, void* stream) {
  if (D_IN <= 0 || D_OUT < 1 || D_OUT > 16 || H < 16 || H > 64 || H % 16 != 0) return -1;
  if (N > 0) {
#define BSC_MLP_EVAL(NCT)                                                                                           \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(k_mlp_eval<NCT>), dim3((N + 15) / 16), dim3(256), 0, (hipStream_t)stream, X, y, \
                     N, D_IN, D_OUT, W, transform, split, err)
    switch (H / 16) {
      case 1: BSC_MLP_EVAL(1); break;
      case 2: BSC_MLP_EVAL(2); break;
      case 3: BSC_MLP_EVAL(3); break;
      default: BSC_MLP_EVAL(4); break;
    }
#undef BSC_MLP_EVAL
  }
  hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, err, err_host);
  return (int)hipGetLastError();
}

// K2c with the same hand-off; S as in bsc_cnn_step
extern "C" int bsc_cnn_eval_rb(const float* X, const int* y, int N, int S, int D_OUT, const double* W, int transform,
                               int split, unsigned int* err, unsigned int* err_host, void* stream) {
  if (S < 1 || S > CNN_SMAX || D_OUT < 1 || D_OUT > 16) return -1;
  static const hipError_t optin =
      hipFuncSetAttribute((const void*)k_cnn_eval, hipFuncAttributeMaxDynamicSharedMemorySize, CNN_DYN_LDS);
  if (optin != hipSuccess) return (int)optin;
  if (N > 0)
    hipLaunchKernelGGL(k_cnn_eval, dim3((N + 15) / 16), dim3(256), CNN_DYN_LDS, (hipStream_t)stream, X, y, N, S, D_OUT,
                       W, transform, split, err);
  hipLaunchKernelGGL(k_eval_finish, dim3(1), dim3(64), 0, (hipStream_t)stream, err, err_host);
  return (int)hipGetLastError();
}

// committee RONI: counters zeroed, k_roni_counts, and the [V, ni + 1] counts' read-back into pinned memory, all on
// `stream`.  ni == 0 scores the base model only (one column).  No verifier or no minibatch slot: nothing is launched
// (the host buffer is not written).
extern "C" int bsc_roni_counts_rb(const float* X, const int* y, long long NX, int D_IN, int D_OUT, const double* W,
                                  const float* U, int n_cand, const long long* rows, const int* nrows, int V, int Bmax,
                                  const int* cand, int ni, int transform, unsigned int* counts,
                                  unsigned int* counts_host, void* stream) {
  if (D_OUT > 16 || D_OUT <= 0 || D_IN <= 0 || ni < 0) return -1;
  if (V <= 0 || Bmax <= 0) return 0;
  const int tiles = (Bmax + 15) / 16;
  if (NX <= 0 || V > 65535 || tiles > 65535 || (ni > 0 && n_cand <= 0)) return -1;
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)V * (ni + 1) * sizeof(unsigned int);
  if (hipMemsetAsync(counts, 0, bytes, s) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_roni_counts, dim3(ni + 1, V, tiles), dim3(256), 0, s, X, y, NX, D_IN, D_OUT, W, U, n_cand, rows,
                     nrows, Bmax, cand, ni, transform, counts);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  return (int)hipMemcpyAsync(counts_host, counts, bytes, hipMemcpyDeviceToHost, s);
}

// logistic scoring: counters zeroed, k_logit_counts, and the [M, 2] counts' read-back into pinned memory, all on
// `stream`.  M models: W and the M - 1 rows of U that sel names.  M == 1 is the evaluation (its priority class);
// more models are a RONI committee.  No row: nothing is launched (the host buffer is not written).
extern "C" int bsc_logit_counts_rb(const double* X, const double* y, int N, int D, int split, const double* W,
                                   const float* U, int n_cand, const int* sel, int M, unsigned int* counts,
                                   unsigned int* counts_host, void* stream) {
  if (D <= 0 || D > LC_DMAX || N < 0 || split < 0 || split > N || M < 1) return -1;
  if (M > 1 && (n_cand <= 0 || U == nullptr || sel == nullptr)) return -1;
  if (N == 0) return 0;
  const int mtiles = (M + LC_MODELS - 1) / LC_MODELS;
  if (mtiles > 65535) return -1;
  hipStream_t s = (hipStream_t)stream;
  const size_t bytes = (size_t)M * 2 * sizeof(unsigned int);
  if (hipMemsetAsync(counts, 0, bytes, s) != hipSuccess) return -1;
  hipLaunchKernelGGL(k_logit_counts, dim3((unsigned int)(((long long)N + LC_ROWS - 1) / LC_ROWS), mtiles),
                     dim3(LC_ROWS), 0, s, X, y, N, D, split, W, U, n_cand, sel, M, M == 1 ? 1 : 0, counts);
  const int rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  return (int)hipMemcpyAsync(counts_host, counts, bytes, hipMemcpyDeviceToHost, s);
}

extern "C" int bsc_noise_table(int nnoisers, int D, unsigned long long seed, float* tbl, void* stream) {
  const long long n = (long long)nnoisers * 100 * D;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_noise_table, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, nnoisers, D, seed, tbl);
  return (int)hipGetLastError();
}

extern "C" int bsc_dp_noise_tbl(const float* delta, int P, int D, const int* noisers, int nn, const float* scale,
                                const float* tbl, int iter_mod, const int* rows, float* noised, void* stream) {
  const long long n = (long long)P * D;
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_dp_noise_tbl, dim3(nblk(n, 256)), dim3(256), 0, (hipStream_t)stream, delta, P, D, noisers,
                     nn, scale, tbl, iter_mod, rows, noised);
  return (int)hipGetLastError();
}

extern "C" int bsc_recover(const long long* ys, int nchunks, int npts, const int* xs, int poly, int d,
                           const double* W, double qscale, double* W_new, long long* coeffs, int* status,
                           void* stream) {
  if (nchunks <= 0) return 0;
  if (npts > 32 || poly > 16) return -1;
  hipLaunchKernelGGL(k_recover, dim3(nblk(nchunks, 64)), dim3(64), 0, (hipStream_t)stream, ys, nchunks, npts, xs,
                     poly, d, W, qscale, W_new, coeffs, status);
  return (int)hipGetLastError();
}

// rstride: int64 elements between consecutive rows of ys (nch * T for a dense [nrows][nch][T] tensor; the
// packed row length when ys are the ranks' partials inside an all_gather buffer, round.hip)
// h_W / h_status (nullable): pinned host mirrors of W_new / status written by the kernel (no read-back copies)
// h_clock (nullable, several ranks): every row's int64 right after its nch x T sums, mirrored to pinned memory
extern "C" int bsc_recover_w_clock(const long long* ys, int nrows, long long rstride, int nch, int T, const int* mask,
                                   const int* ycols, const int* xs, int npts, const long long* A, const int* basis,
                                   int poly, int shift, unsigned long long inv_lo, unsigned long long inv_hi, int d,
                                   const double* W, double qscale, double* W_new, long long* coeffs, int* status,
                                   long long* agg_out, double* h_W, int* h_status, long long* h_clock, void* stream) {
  if (nch <= 0) return 0;
  if (npts > RW_MAXP || poly > RW_MAXC || poly > npts || shift < 0 || shift > 100 || nrows <= 0) return -1;
  if (rstride < (long long)nch * T || (h_clock != nullptr && (nrows > 256 || rstride < (long long)nch * T + 1)))
    return -1;
  hipLaunchKernelGGL(k_recover_w, dim3(nblk(nch, RW_CPB)), dim3(256), 0, (hipStream_t)stream, ys, nrows, rstride, nch,
                     T, mask, ycols, xs, npts, A, basis, poly, shift, inv_lo, inv_hi, d, W, qscale, W_new, coeffs,
                     status, agg_out, h_W, h_status, h_clock);
  return (int)hipGetLastError();
}

extern "C" int bsc_add_rows(const float* delta, int D, const int* rows, int nrows, const double* W, double* W_new,
                            void* stream) {
  if (D <= 0) return 0;
  hipLaunchKernelGGL(k_add_rows, dim3(nblk(D, 256)), dim3(256), 0, (hipStream_t)stream, delta, D, rows, nrows, W,
                     W_new);
  return (int)hipGetLastError();
}
