// Fused brain head (the arithmetic the reference itself owns):
//   hidden --LN1--> sum_s w[b,s]*(.) --LN2--> dropout --Linear(E->V)--> pred ; loss = MSE + lambda*||W||^2
// reference: src/litmodule/videollama2_vlb_litmodule.py:245-254,302 ; src/utils.py:56,66-71.
// Opt-in objectives in place of the MSE (its docstring :290-301): 1 - mean_b cos(pred_b, y_b), plain or row-centred (Pearson).
//
// HBM-bound.  The LN1-normalised [B,S,E] tensor is never materialised: because LN1's affine is
// per-column,   pooled[e] = g1[e] * sum_s w_s*rstd_s*(x_se - mu_s) + b1[e] * sum_s w_s,
// so one pass over `hidden` with per-token (mu, rstd) suffices, and tokens whose HRF weight is zero
// (the prompt, instruction and padding spans) are skipped altogether.
// All cross-block reductions go through partial slabs summed in a fixed order (bitwise reproducible).
#include "common.hpp"

namespace {

constexpr int POOL_ROWS = 32;     // tokens per pooling block (8 waves x 4 tokens)
constexpr int RIDGE_ROWS = 16;    // ridge rows per block (4 waves x 4 rows)
constexpr int BMAX = 8;           // clips handled per pass by the ridge kernels
constexpr int DZ_SPLIT = 32;      // V-splits of the dz reduction

__device__ __forceinline__ void ld8(const bf16* p, float (&v)[8]) {
  const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
}

// ---------------------------------------------------------------- forward 1: LN1 stats + weighted pool
template <int NI>   // NI = ceil(E/512) chunks of 8 columns per lane
__global__ __launch_bounds__(512) void head_pool_kernel(const bf16* __restrict__ hidden, const float* __restrict__ wmask,
                                                        float* __restrict__ partial, float* __restrict__ stats, int S,
                                                        int E, float eps, const int* __restrict__ cu) {
  extern __shared__ __attribute__((aligned(16))) float red[];   // [4][E]
  const int b = blockIdx.y, blk = blockIdx.x, nblk = gridDim.x;
  // packed hidden: clip b = rows [cu[b], cu[b+1]); wmask / stats stay dense [B,S]
  const int Sb = cu ? cu[b + 1] - cu[b] : S;
  const int64_t row0 = cu ? cu[b] : (int64_t)b * S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float acc[NI][8];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
  float sw = 0.f;
  // this wave's tokens: blk*32 + wave + {0,8,16,24}; rows with zero weight are skipped (wave-uniform).
  // Software pipeline: the next live row is in flight (raw bf16) while the current one is reduced.
  auto load_row = [&](int s_, bf16x8 (&dst)[NI]) {
    const bf16* xr = hidden + (row0 + s_) * E;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = lane * 8 + i * 512;
      dst[i] = c < E ? *reinterpret_cast<const bf16x8*>(xr + c) : bf16x8{};
    }
  };
  int live[POOL_ROWS / 8];
  float wl[POOL_ROWS / 8];
  int nlive = 0;
#pragma unroll
  for (int q = 0; q < POOL_ROWS / 8; ++q) {
    const int s_ = blk * POOL_ROWS + wave + 8 * q;
    const float w_ = s_ < Sb ? wmask[(int64_t)b * S + s_] : 0.f;
    if (w_ != 0.f) { live[nlive] = s_; wl[nlive] = w_; ++nlive; }
  }
  bf16x8 cur[NI], nxt[NI];
  if (nlive > 0) load_row(live[0], cur);
#pragma unroll
  for (int q = 0; q < POOL_ROWS / 8; ++q) {
    if (q >= nlive) break;
    if (q + 1 < nlive) load_row(live[q + 1], nxt);
    const int s = live[q];
    const float w = wl[q];
    float x[NI][8];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) { x[i][j] = (float)cur[i][j]; sum += x[i][j]; }
    const float mu = wave_sum(sum) / E;
    float var = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = lane * 8 + i * 512;
      if (c < E) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = x[i][j] - mu; var += d * d; }
      }
    }
    const float rstd = rsqrtf(wave_sum(var) / E + eps);
    const float a = w * rstd;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] += a * (x[i][j] - mu);
    sw += w;
    if (lane == 0) { stats[((int64_t)b * S + s) * 2] = mu; stats[((int64_t)b * S + s) * 2 + 1] = rstd; }
#pragma unroll
    for (int i = 0; i < NI; ++i) cur[i] = nxt[i];
  }
  // deterministic tree reduction over the 8 waves through LDS
  for (int stride = 4; stride >= 1; stride >>= 1) {
    if (wave >= stride && wave < 2 * stride) {
      float* dst = red + (wave - stride) * E;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int c = lane * 8 + i * 512;
        if (c < E) {
          *reinterpret_cast<f32x4*>(dst + c) = f32x4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
          *reinterpret_cast<f32x4*>(dst + c + 4) = f32x4{acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
        }
      }
      if (lane == 0) red[4 * E + (wave - stride)] = sw;
    }
    __syncthreads();
    if (wave < stride) {
      const float* src = red + wave * E;
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int c = lane * 8 + i * 512;
        if (c < E) {
          const f32x4 lo = *reinterpret_cast<const f32x4*>(src + c), hi = *reinterpret_cast<const f32x4*>(src + c + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { acc[i][j] += lo[j]; acc[i][4 + j] += hi[j]; }
        }
      }
      sw += red[4 * E + wave];
    }
    __syncthreads();
  }
  if (wave == 0) {
    float* dst = partial + ((int64_t)b * nblk + blk) * (E + 2);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int c = lane * 8 + i * 512;
      if (c < E) {
#pragma unroll
        for (int j = 0; j < 8; ++j) dst[c + j] = acc[i][j];
      }
    }
    if (lane == 0) dst[E] = sw;
  }
}

// ---------------------------------------------------------------- forward 2a: sum the pooling slabs (fixed order)
// grid (ceil(E/256), B): thread e sums partial[b][0..nblk)[e]; thread 0 of block x=0 sums the weights.
__global__ __launch_bounds__(256) void head_reduce_kernel(const float* __restrict__ partial, int nblk,
                                                          float* __restrict__ pooled_raw, float* __restrict__ sumw, int E) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  const float* pb = partial + (int64_t)b * nblk * (E + 2);
  if (e < E) {
    float raw = 0.f;
#pragma unroll 8
    for (int k = 0; k < nblk; ++k) raw += pb[(int64_t)k * (E + 2) + e];
    pooled_raw[(int64_t)b * E + e] = raw;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    float sw = 0.f;
    for (int k = 0; k < nblk; ++k) sw += pb[(int64_t)k * (E + 2) + E];
    sumw[b] = sw;
  }
}
// ---------------------------------------------------------------- forward 2b: LN1 affine, LN2, dropout -> z (bf16)
__global__ __launch_bounds__(1024) void head_ln2_kernel(const float* __restrict__ pooled_raw, const float* __restrict__ sumw,
                                                        const bf16* __restrict__ g1, const bf16* __restrict__ b1,
                                                        const bf16* __restrict__ g2, const bf16* __restrict__ b2,
                                                        const float* __restrict__ keep, float* __restrict__ zhat,
                                                        float* __restrict__ ln2_rstd, bf16* __restrict__ z, int E, float eps) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  const float sw = sumw[b];
  float lsum = 0.f;
  for (int e = threadIdx.x; e < E; e += blockDim.x)
    lsum += (float)g1[e] * pooled_raw[(int64_t)b * E + e] + (float)b1[e] * sw;
  const float mean = block_sum(lsum, red) / E;
  float lvar = 0.f;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    const float pv = (float)g1[e] * pooled_raw[(int64_t)b * E + e] + (float)b1[e] * sw;
    lvar += (pv - mean) * (pv - mean);
  }
  const float rstd = rsqrtf(block_sum(lvar, red) / E + eps);
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    const float pv = (float)g1[e] * pooled_raw[(int64_t)b * E + e] + (float)b1[e] * sw;
    const float zh = (pv - mean) * rstd;
    zhat[(int64_t)b * E + e] = zh;
    float zz = zh * (float)g2[e] + (float)b2[e];
    if (keep) zz *= keep[(int64_t)b * E + e];
    z[(int64_t)b * E + e] = (bf16)zz;
  }
  if (threadIdx.x == 0) ln2_rstd[b] = rstd;
}

// ---------------------------------------------------------------- feature cache: scatter / gather of (pooled_raw, sumw)
// Everything downstream of head_reduce_kernel reads only pooled_raw [B,E] and sumw [B], so a frozen backbone's clip is
// fully described by those two; they are stored per clip in cache rows [N,E] / [N] and copied back verbatim (fp32, no
// arithmetic).  grid (ceil(E/256), B).  rows[b] < 0 skips position b; a row outside [0, n_rows) is never touched (the
// host checks the indices before it uploads them, this is a second guard).
__global__ __launch_bounds__(256) void feature_cache_store_kernel(const float* __restrict__ pooled_raw,
                                                                  const float* __restrict__ sumw, const int* __restrict__ rows,
                                                                  float* __restrict__ cache_pooled, float* __restrict__ cache_sumw,
                                                                  int E, int n_rows) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  const int r = rows[b];
  if (r < 0 || r >= n_rows) return;
  if (e < E) cache_pooled[(int64_t)r * E + e] = pooled_raw[(int64_t)b * E + e];
  if (blockIdx.x == 0 && threadIdx.x == 0) cache_sumw[r] = sumw[b];
}
__global__ __launch_bounds__(256) void feature_cache_gather_kernel(const float* __restrict__ cache_pooled,
                                                                   const float* __restrict__ cache_sumw, const int* __restrict__ rows,
                                                                   float* __restrict__ pooled_raw, float* __restrict__ sumw, int E,
                                                                   int n_rows) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  const int r = rows[b];
  if (r < 0 || r >= n_rows) return;
  if (e < E) pooled_raw[(int64_t)b * E + e] = cache_pooled[(int64_t)r * E + e];
  if (blockIdx.x == 0 && threadIdx.x == 0) sumw[b] = cache_sumw[r];
}

// ================================================================ the ridge layer: one head, or G heads, one per subject
// Plain head: W [V, E], bias [V].  Per-subject heads: W [G*V, E], bias [G*V], group[b] in [0, G) names the
// head of clip b; pred / y stay [B, V]:   pred[b, v] = W[group[b]*V + v, :] . z[b, :] + bias[group[b]*V + v].
// Every ridge kernel is ONE template with a compile-time GROUPED.  GROUPED splits the row index into (head g, row v of the
// head) and lets a clip take part only in its own head's rows; !GROUPED fixes g = 0, row = v, every clip takes part, and
// `group` is never read (the plain entries pass nullptr).  A clip's chain of additions is the same in both, the blocks /
// tiles of head g come in the plain order behind those of the heads before it, and the (sum err^2, sum W^2) partials keep
// one pair per block: with G = 1 the grouped instantiation gives the plain one's bits.

// ---------------------------------------------------------------- forward 3: ridge GEMV + loss partials
// grid G * bpg, bpg = ceil(V/RIDGE_ROWS): block -> (g, RIDGE_ROWS rows of head g) = 4 waves x RIDGE_ROWS/4 rows of W; z (bf16
// [<=BMAX, E]) is staged once per block into LDS and re-read from there for every row (the W stream, 16-byte lanes, is the
// only HBM traffic).
template <bool GROUPED>
__global__ __launch_bounds__(256) void ridge_fwd_kernel(const bf16* __restrict__ W, const bf16* __restrict__ bias,
                                                        const bf16* __restrict__ z, const float* __restrict__ y,
                                                        const int* __restrict__ group, float* __restrict__ pred,
                                                        float* __restrict__ lpart, int B, int E, int V, int bpg) {
  extern __shared__ __attribute__((aligned(16))) char zsm[];     // [nb][E] bf16
  __shared__ float red[8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = GROUPED ? blockIdx.x / bpg : 0, vb = GROUPED ? blockIdx.x % bpg : blockIdx.x;   // head, block of rows inside it
  float mse = 0.f, w2 = 0.f;
  for (int b0 = 0; b0 < B; b0 += BMAX) {
    const int nb = min(BMAX, B - b0);
    __syncthreads();
    for (int i = threadIdx.x * 8; i < nb * E; i += 256 * 8)
      *reinterpret_cast<bf16x8*>(zsm + (int64_t)i * 2) = *reinterpret_cast<const bf16x8*>(z + (int64_t)b0 * E + i);
    __syncthreads();
    bool mine[BMAX];
#pragma unroll
    for (int i = 0; i < BMAX; ++i) {
      mine[i] = i < nb;
      if constexpr (GROUPED) mine[i] = mine[i] && group[b0 + i] == g;
    }
    for (int rr = 0; rr < RIDGE_ROWS / 4; ++rr) {
      const int v = vb * RIDGE_ROWS + wave * (RIDGE_ROWS / 4) + rr;
      if (v >= V) break;
      const int64_t row = (int64_t)g * V + v;
      const bf16* wr = W + row * E;
      float acc[BMAX];
#pragma unroll
      for (int i = 0; i < BMAX; ++i) acc[i] = 0.f;
#pragma unroll 4
      for (int c = lane * 8; c < E; c += 512) {
        float w[8]; ld8(wr + c, w);
        if (b0 == 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) w2 += w[j] * w[j];
        }
#pragma unroll
        for (int i = 0; i < BMAX; ++i) {
          if (mine[i]) {
            float zz[8]; ld8(reinterpret_cast<const bf16*>(zsm) + (int64_t)i * E + c, zz);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i] += w[j] * zz[j];
          }
        }
      }
#pragma unroll
      for (int i = 0; i < BMAX; ++i) {
        if (mine[i]) {
          const float pv = wave_sum(acc[i]) + (float)bias[row];
          if (lane == 0) {
            pred[(int64_t)(b0 + i) * V + v] = pv;
            const float d = y ? pv - y[(int64_t)(b0 + i) * V + v] : 0.f;
            mse += d * d;
          }
        }
      }
    }
  }
  w2 = wave_sum(w2);
  if (lane == 0) { red[wave] = mse; red[4 + wave] = w2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    lpart[blockIdx.x * 2] = red[0] + red[1] + red[2] + red[3];
    lpart[blockIdx.x * 2 + 1] = red[4] + red[5] + red[6] + red[7];
  }
}
// ---------------------------------------------------------------- forward 3 (MFMA form, E <= 4096, E % 128 == 0, B <= 16)
// pred[b, v] = sum_e z[b,e] W[v,e]: a skinny contraction (M = B <= 16) -> v_mfma_f32_16x16x32_bf16 with the
// MFMA rows = 16 rows of W and the MFMA columns = clips.  Each of the 4 waves of a block owns one QUARTER
// of E and keeps its z fragments in registers for the whole kernel (<= 128 VGPRs), so the only memory
// stream is W: 32 independent 1-KiB fragment loads per wave per row tile.  Blocks are persistent over
// row tiles; the four K-quarters are summed through LDS; sum(W^2) and the squared error ride along.
// The ntiles = G * tpg row tiles, tpg = ceil(V/16): tile t is rows [16 tl, 16 tl + 16) of head g = t / tpg, tl = t % tpg - a
// tile never spans two heads, the last tile of a head clamps its rows to the head's own last row.  All 16 clip columns are
// contracted with every tile (no extra matrix work per head: the W stream is the cost); the epilogue keeps column b only
// where group[b] == g.  sum W^2 counts every live row of every tile.
template <int KSTEPS, bool GROUPED>   // KSTEPS = E / 128: k-steps of 32 per wave
__global__ __launch_bounds__(256) void ridge_fwd_mfma_kernel(const bf16* __restrict__ W, const bf16* __restrict__ bias,
                                                             const bf16* __restrict__ z, const float* __restrict__ y,
                                                             const int* __restrict__ group, float* __restrict__ pred,
                                                             float* __restrict__ lpart, int B, int E, int V, int tpg,
                                                             int ntiles) {
  __shared__ float red[3][4][64];
  __shared__ float lred[8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int kq = wave * KSTEPS * 32;                       // first column of this wave's quarter
  // B operand: lane holds z[b = fr][kq + 32*s + 8*fq .. +8]  (zero rows for b >= B)
  bf16x8 zf[KSTEPS];
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s) {
    zf[s] = bf16x8{};
    if (fr < B) zf[s] = *reinterpret_cast<const bf16x8*>(z + (int64_t)fr * E + kq + 32 * s + 8 * fq);
  }
  int myg = 0;                                             // head of this lane's clip column
  if constexpr (GROUPED) myg = fr < B ? group[fr] : -1;
  float mse = 0.f, w2 = 0.f;
  for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int g = GROUPED ? t / tpg : 0, tl = GROUPED ? t % tpg : t;
    const int v = min(tl * 16 + fr, V - 1);
    const bf16* wr = W + ((int64_t)g * V + v) * E + kq + 8 * fq;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool count = tl * 16 + fr < V;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) {
      const bf16x8 wf = *reinterpret_cast<const bf16x8*>(wr + 32 * s);
      if (count) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = (float)wf[j]; w2 += f * f; }
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, zf[s], acc, 0, 0, 0);
    }
    __syncthreads();                                       // red[] free again
    if (wave > 0) {
#pragma unroll
      for (int e = 0; e < 4; ++e) red[wave - 1][e][lane] = acc[e];
    }
    __syncthreads();
    if (wave == 0 && (GROUPED ? myg == g : fr < B)) {
      // lane holds clip b = fr (of head g), rows v = tl*16 + 4*fq + e of that head
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int vv = tl * 16 + 4 * fq + e;
        if (vv < V) {
          const float pv = acc[e] + red[0][e][lane] + red[1][e][lane] + red[2][e][lane] + (float)bias[(int64_t)g * V + vv];
          pred[(int64_t)fr * V + vv] = pv;
          const float d = y ? pv - y[(int64_t)fr * V + vv] : 0.f;
          mse += d * d;
        }
      }
    }
  }
  mse = wave_sum(mse);
  w2 = wave_sum(w2);
  if (lane == 0) { lred[wave] = mse; lred[4 + wave] = w2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    lpart[blockIdx.x * 2] = lred[0] + lred[1] + lred[2] + lred[3];
    lpart[blockIdx.x * 2 + 1] = lred[4] + lred[5] + lred[6] + lred[7];
  }
}

// one block: thread i sums entries i, i+256, ... in order; the 256 partials are then tree-summed in LDS
// (fixed order -> reproducible)
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ lpart, int nblk, float inv_bv, float lambda,
                                                            float* __restrict__ out) {
  __shared__ double sm[2][256];
  double mse = 0.0, w2 = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) { mse += lpart[2 * i]; w2 += lpart[2 * i + 1]; }
  sm[0][threadIdx.x] = mse; sm[1][threadIdx.x] = w2;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) { sm[0][threadIdx.x] += sm[0][threadIdx.x + s2]; sm[1][threadIdx.x] += sm[1][threadIdx.x + s2]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = (float)(sm[0][0] * inv_bv);
    out[1] = (float)(lambda * sm[1][0]);
    out[2] = out[0] + out[1];
  }
}

// ---------------------------------------------------------------- correlation objectives (cosine / pearson), forward
// Reference: the training_step docstring of src/litmodule/videollama2_vlb_litmodule.py:290-301 names
//   1 - F.cosine_similarity(brain_encoding, y, dim=-1).mean() + l2_reg ;  pearson is the same on row-centred inputs.
// Row statistics, one block of 1024 per clip: rowstat[b] = {mu_p, mu_y, sum u^2, sum t^2, sum u t, c_b, 0, 0} with
// u = p - mu_p, t = y - mu_y (mu = 0 for cosine: the mean pass is skipped).  Two passes (means, then centred sums), so a
// common offset of the rows costs nothing.  A row of [B,V] fp32 starts at element b*V, 16-byte aligned only when that is a
// multiple of 4: up to 3 head elements one per thread, f32x4 body, up to 3 tail elements; when pred and y rows differ in
// alignment everything goes the scalar way.  A thread adds head, body, tail in that order into one accumulator per
// quantity; block_sum is wave_sum + the 16 wave partials in order: fixed order, no atomics.
__device__ __forceinline__ void row_split(const float* p, const float* q, int V, int& head, int& nvec) {
  const uintptr_t ap = reinterpret_cast<uintptr_t>(p), aq = reinterpret_cast<uintptr_t>(q);
  if ((ap & 15) != (aq & 15)) { head = V; nvec = 0; return; }        // scalar throughout
  head = (int)(((16 - (ap & 15)) & 15) >> 2);
  if (head > V) head = V;
  nvec = (V - head) >> 2;
}

template <bool CENTRE>
__global__ __launch_bounds__(1024) void head_rowstat_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                            float* __restrict__ rowstat, int V) {
  __shared__ float red[16];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* pr = pred + (int64_t)b * V;
  const float* yr = y + (int64_t)b * V;
  int head, nvec;
  row_split(pr, yr, V, head, nvec);
  const int tail0 = head + 4 * nvec;             // first tail element
  float mp = 0.f, my = 0.f;
  if constexpr (CENTRE) {
    float sp = 0.f, sy = 0.f;
    for (int i = tid; i < head; i += 1024) { sp += pr[i]; sy += yr[i]; }
    for (int k = tid; k < nvec; k += 1024) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(pr + head + 4 * k), c = *reinterpret_cast<const f32x4*>(yr + head + 4 * k);
#pragma unroll
      for (int j = 0; j < 4; ++j) { sp += a[j]; sy += c[j]; }
    }
    for (int i = tail0 + tid; i < V; i += 1024) { sp += pr[i]; sy += yr[i]; }
    mp = block_sum(sp, red) / V;
    my = block_sum(sy, red) / V;
  }
  float suu = 0.f, stt = 0.f, sut = 0.f;
  for (int i = tid; i < head; i += 1024) {
    const float u = pr[i] - mp, t = yr[i] - my;
    suu += u * u; stt += t * t; sut += u * t;
  }
  for (int k = tid; k < nvec; k += 1024) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(pr + head + 4 * k), c = *reinterpret_cast<const f32x4*>(yr + head + 4 * k);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float u = a[j] - mp, t = c[j] - my;
      suu += u * u; stt += t * t; sut += u * t;
    }
  }
  for (int i = tail0 + tid; i < V; i += 1024) {
    const float u = pr[i] - mp, t = yr[i] - my;
    suu += u * u; stt += t * t; sut += u * t;
  }
  suu = block_sum(suu, red);
  stt = block_sum(stt, red);
  sut = block_sum(sut, red);
  if (tid == 0) {
    const float nu = fmaxf(sqrtf(suu), 1e-8f), nt = fmaxf(sqrtf(stt), 1e-8f);      // F.cosine_similarity's clamp
    float* o = rowstat + (int64_t)b * 8;
    o[0] = mp; o[1] = my; o[2] = suu; o[3] = stt; o[4] = sut; o[5] = sut / (nu * nt); o[6] = 0.f; o[7] = 0.f;
  }
}

// loss_finalize_kernel for the correlation objectives: the same sums over lpart (so out[1] has the bits loss_finalize_kernel
// gave it), the data term 1 - mean_b c_b from rowstat summed in clip order in double, and the plain MSE the ridge forward
// accumulated anyway -> aux[0] (aux[1] = mean_b c_b).
__global__ __launch_bounds__(256) void loss_finalize_corr_kernel(const float* __restrict__ lpart, int nblk, float inv_bv, float lambda,
                                                                 const float* __restrict__ rowstat, int B, float* __restrict__ out,
                                                                 float* __restrict__ aux) {
  __shared__ double sm[2][256];
  double mse = 0.0, w2 = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) { mse += lpart[2 * i]; w2 += lpart[2 * i + 1]; }
  sm[0][threadIdx.x] = mse; sm[1][threadIdx.x] = w2;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) { sm[0][threadIdx.x] += sm[0][threadIdx.x + s2]; sm[1][threadIdx.x] += sm[1][threadIdx.x + s2]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double cs = 0.0;
    for (int b = 0; b < B; ++b) cs += rowstat[(int64_t)b * 8 + 5];
    cs /= B;
    out[0] = (float)(1.0 - cs);
    out[1] = (float)(lambda * sm[1][0]);
    out[2] = out[0] + out[1];
    aux[0] = (float)(sm[0][0] * inv_bv);
    aux[1] = (float)cs;
  }
}

// backward of the correlation objectives, first launch: coef[b] = {a_b, b_b, mu_p, mu_y} from rowstat and loss_scale,
//   b_b = -s / (B nu nt),  a_b = s c_b / (B nu ||u||)  (0 where ||u|| = 0).  Where the norm is not clamped that is
// s c_b / (B nu^2).  Under the clamp it is what autograd gives for F.cosine_similarity, which clamps the norm's VALUE under
// no_grad and differentiates the norm itself: the kernels follow autograd there, not the derivative of the clamped function.
__global__ void head_loss_coef_kernel(const float* __restrict__ rowstat, float* __restrict__ coef, int B, float loss_scale) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const float* r = rowstat + (int64_t)b * 8;
  const float ru = sqrtf(r[2]), nu = fmaxf(ru, 1e-8f), nt = fmaxf(sqrtf(r[3]), 1e-8f);
  const float sb = loss_scale / (float)B;
  coef[4 * b] = ru > 0.f ? sb * r[5] / (nu * ru) : 0.f;
  coef[4 * b + 1] = -sb / (nu * nt);
  coef[4 * b + 2] = r[0];
  coef[4 * b + 3] = r[1];
}

// d pred of the correlation objectives (CORR forms of the three kernels below): coef[b] = {a_b, b_b, mu_p, mu_y}, filled by
// head_loss_coef_kernel;  d pred[b,v] = a_b (p - mu_p) + b_b (y - mu_y).  The centred form: rows may sit on a large offset.
__device__ __forceinline__ float dpred_corr(const float* __restrict__ coef, int b, float p, float yv) {
  const float* c = coef + 4 * b;
  return c[0] * (p - c[2]) + c[1] * (yv - c[3]);
}

// ================================================================ per-target loss weights and masks
// tw fp32 [H,V], H = max(1,G), every value finite and >= 0: clip b reads the row of its head, w_v = tw[group[b], v] (group
// NULL: row 0).  Per clip  W_b = sum w,  m_b = sum w (p-y)^2 / W_b,  and for cosine / pearson  u = p - mu_p, t = y - mu_y with
// mu = sum w (.) / W_b (0 for cosine),  S_uu = sum w u^2, S_tt = sum w t^2, S_ut = sum w u t,
// c_b = S_ut / (max(sqrt S_uu, 1e-8) max(sqrt S_tt, 1e-8)).  A target with w_v = 0 is SELECTED away, never multiplied away:
// pred and y there are loaded but enter no arithmetic, so NaN / Inf in a masked y changes no bit of any result.
// The row walk is head_rowstat_kernel's (head, f32x4 body, tail; fixed-order block_sum, no atomics) over three rows.
__device__ __forceinline__ void row_split3(const float* p, const float* q, const float* r, int V, int& head, int& nvec) {
  const uintptr_t ap = reinterpret_cast<uintptr_t>(p), aq = reinterpret_cast<uintptr_t>(q), ar = reinterpret_cast<uintptr_t>(r);
  if ((ap & 15) != (aq & 15) || (ap & 15) != (ar & 15)) { head = V; nvec = 0; return; }   // scalar throughout
  head = (int)(((16 - (ap & 15)) & 15) >> 2);
  if (head > V) head = V;
  nvec = (V - head) >> 2;
}

// f(w, p, y) over one row in the fixed order: head one element per thread, f32x4 body, tail
template <typename F>
__device__ __forceinline__ void wrow_walk(const float* __restrict__ wr, const float* __restrict__ pr, const float* __restrict__ yr,
                                          int V, int head, int nvec, F&& f) {
  const int tid = threadIdx.x, tail0 = head + 4 * nvec;
  for (int i = tid; i < head; i += 1024) f(wr[i], pr[i], yr[i]);
  for (int k = tid; k < nvec; k += 1024) {
    const f32x4 w = *reinterpret_cast<const f32x4*>(wr + head + 4 * k), a = *reinterpret_cast<const f32x4*>(pr + head + 4 * k),
                c = *reinterpret_cast<const f32x4*>(yr + head + 4 * k);
#pragma unroll
    for (int j = 0; j < 4; ++j) f(w[j], a[j], c[j]);
  }
  for (int i = tail0 + tid; i < V; i += 1024) f(wr[i], pr[i], yr[i]);
}

// one block of 1024 per clip -> wstat[b] = {mu_p, mu_y, S_uu, S_tt, S_ut, c_b, W_b, m_b}  (mse: slots 0-5 are 0).
// pearson takes two passes (W_b and the weighted means, then the centred sums); mse and cosine take one.
template <int KIND>
__global__ __launch_bounds__(1024) void head_wrowstat_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                             const float* __restrict__ tw, const int* __restrict__ group,
                                                             float* __restrict__ wstat, int V) {
  constexpr bool CENTRE = KIND == VLB_LOSS_PEARSON, CORRK = KIND != VLB_LOSS_MSE;
  __shared__ float red[16];
  const int b = blockIdx.x;
  const float* pr = pred + (int64_t)b * V;
  const float* yr = y + (int64_t)b * V;
  const float* wr = tw + (int64_t)(group ? group[b] : 0) * V;
  int head, nvec;
  row_split3(pr, yr, wr, V, head, nvec);
  float sw = 0.f, mp = 0.f, my = 0.f;
  if constexpr (CENTRE) {
    float sp = 0.f, sy = 0.f;
    wrow_walk(wr, pr, yr, V, head, nvec, [&](float w, float p, float yv) {
      if (w > 0.f) { sw += w; sp += w * p; sy += w * yv; }
    });
    sw = block_sum(sw, red);
    mp = block_sum(sp, red) / sw;
    my = block_sum(sy, red) / sw;
  }
  float suu = 0.f, stt = 0.f, sut = 0.f, sm = 0.f;
  wrow_walk(wr, pr, yr, V, head, nvec, [&](float w, float p, float yv) {
    if (w > 0.f) {
      if constexpr (!CENTRE) sw += w;
      const float d = p - yv;
      sm += w * d * d;
      if constexpr (CORRK) {
        const float u = p - mp, t = yv - my;
        suu += w * u * u; stt += w * t * t; sut += w * u * t;
      }
    }
  });
  if constexpr (!CENTRE) sw = block_sum(sw, red);
  sm = block_sum(sm, red);
  if constexpr (CORRK) {
    suu = block_sum(suu, red);
    stt = block_sum(stt, red);
    sut = block_sum(sut, red);
  }
  if (threadIdx.x == 0) {
    float* o = wstat + (int64_t)b * 8;
    float cb = 0.f;
    if constexpr (CORRK) {
      const float nu = fmaxf(sqrtf(suu), 1e-8f), nt = fmaxf(sqrtf(stt), 1e-8f);      // F.cosine_similarity's clamp
      cb = sut / (nu * nt);
    }
    o[0] = mp; o[1] = my; o[2] = suu; o[3] = stt; o[4] = sut; o[5] = cb; o[6] = sw; o[7] = sm / sw;
  }
}

// one block: sum W^2 from the ridge forward's partials exactly as loss_finalize_kernel sums it (out[1] keeps the bits the
// plain forward wrote); the forward's sum (pred-y)^2 partials are NOT read (masked targets may have put NaN there).  The
// data term from wstat, clips summed in order in double: out[0] = mean_b m_b (corr = 0) or 1 - mean_b c_b; aux = both means.
__global__ __launch_bounds__(256) void wloss_finalize_kernel(const float* __restrict__ lpart, int nblk, float lambda,
                                                             const float* __restrict__ wstat, int B, int corr,
                                                             float* __restrict__ out, float* __restrict__ aux) {
  __shared__ double sm[256];
  double w2 = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) w2 += lpart[2 * i + 1];
  sm[threadIdx.x] = w2;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) sm[threadIdx.x] += sm[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double ms = 0.0, cs = 0.0;
    for (int b = 0; b < B; ++b) { ms += wstat[(int64_t)b * 8 + 7]; cs += wstat[(int64_t)b * 8 + 5]; }
    ms /= B; cs /= B;
    out[0] = (float)(corr ? 1.0 - cs : ms);
    out[1] = (float)(lambda * sm[0]);
    out[2] = out[0] + out[1];
    aux[0] = (float)ms;
    aux[1] = (float)cs;
  }
}

// d pred fp32 [B,V] of the weighted objective, grid (ceil(V/256), B):
//   mse:  s 2 w (p - y) / (B W_b);   cosine / pearson:  w (a_b (p - mu_p) + b_b (y - mu_y)),
// a_b, b_b the expressions of head_loss_coef_kernel on the weighted sums; exactly 0 where w = 0 (y is not read there).
template <int KIND>
__global__ __launch_bounds__(256) void head_wdpred_kernel(const float* __restrict__ pred, const float* __restrict__ y,
                                                          const float* __restrict__ tw, const int* __restrict__ group,
                                                          const float* __restrict__ wstat, float* __restrict__ dpred, int B, int V,
                                                          float loss_scale) {
  const int b = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const float* r = wstat + (int64_t)b * 8;
  const float w = tw[(int64_t)(group ? group[b] : 0) * V + v];
  float dp = 0.f;
  if (w > 0.f) {
    const float p = pred[(int64_t)b * V + v], yv = y[(int64_t)b * V + v];
    if constexpr (KIND == VLB_LOSS_MSE) {
      const float cm = loss_scale * 2.f / ((float)B * r[6]);
      dp = cm * w * (p - yv);
    } else {
      const float ru = sqrtf(r[2]), nu = fmaxf(ru, 1e-8f), nt = fmaxf(sqrtf(r[3]), 1e-8f);
      const float sb = loss_scale / (float)B;
      const float ca = ru > 0.f ? sb * r[5] / (nu * ru) : 0.f, cb = -sb / (nu * nt);
      dp = w * (ca * (p - r[0]) + cb * (yv - r[1]));
    }
  }
  dpred[(int64_t)b * V + v] = dp;
}

// d pred of clip b at row v of ITS head, the one spelling for both objectives (the other heads' rows see 0 for this clip):
// gscale * (pred - y), or the correlation form above.
// CORR is a three-way mode naming where d pred comes from: DP_MSE and DP_CORR derive it from (pred, y); DP_BUF reads it
// from a finished fp32 [B,V] buffer handed in where the other two take `pred` (head_wdpred_kernel wrote it; y and coef are
// not read).
enum : int { DP_MSE = 0, DP_CORR = 1, DP_BUF = 2 };
template <int CORR>
__device__ __forceinline__ float dpred_own(const float* __restrict__ pred, const float* __restrict__ y, int b, int v, int V,
                                           float gscale, const float* __restrict__ coef) {
  if constexpr (CORR == DP_BUF) return pred[(int64_t)b * V + v];
  else if constexpr (CORR == DP_CORR) return dpred_corr(coef, b, pred[(int64_t)b * V + v], y[(int64_t)b * V + v]);
  else return gscale * (pred[(int64_t)b * V + v] - y[(int64_t)b * V + v]);
}

// d pred^T over all GV = G*V rows as the skinny-wgrad G operand: dpT[g*V + v, b] = d pred[b, v] for b < B (and, GROUPED,
// group[b] == g), else 0 - the columns b < 16 are all written
template <int CORR, bool GROUPED>
__global__ void dpred_t_kernel(const float* __restrict__ pred, const float* __restrict__ y, const int* __restrict__ group,
                               bf16* __restrict__ dpT, int B, int V, int64_t GV, float gscale, const float* __restrict__ coef) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= GV * 16) return;
  const int64_t row = i >> 4;
  const int b = (int)(i & 15), g = GROUPED ? (int)(row / V) : 0, v = GROUPED ? (int)(row % V) : (int)row;
  bool mine = b < B;
  if constexpr (GROUPED) mine = mine && group[b] == g;
  dpT[i] = (bf16)(mine ? dpred_own<CORR>(pred, y, b, v, V, gscale, coef) : 0.f);
}

// ---------------------------------------------------------------- backward 1: dW, dbias   (z staged in LDS)
// grid G * bpg as ridge_fwd_kernel, one row of dW per (g, v).  A clip of another head adds nothing to the row: it is skipped,
// so a head without a clip gets the fp32 product l2coef * W and dbias = 0 exactly.
template <int CORR, bool GROUPED>
__global__ __launch_bounds__(256) void ridge_bwd_w_kernel(const bf16* __restrict__ W, const bf16* __restrict__ z,
                                                          const float* __restrict__ pred, const float* __restrict__ y,
                                                          const int* __restrict__ group, float* __restrict__ dW,
                                                          float* __restrict__ dbias, int B, int E, int V, int bpg, float gscale,
                                                          float l2coef, const float* __restrict__ coef) {
  extern __shared__ __attribute__((aligned(16))) char zsm[];     // [nb][E] bf16
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = GROUPED ? blockIdx.x / bpg : 0, vb = GROUPED ? blockIdx.x % bpg : blockIdx.x;
  for (int b0 = 0; b0 < B; b0 += BMAX) {
    const int nb = min(BMAX, B - b0);
    __syncthreads();
    for (int i = threadIdx.x * 8; i < nb * E; i += 256 * 8)
      *reinterpret_cast<bf16x8*>(zsm + (int64_t)i * 2) = *reinterpret_cast<const bf16x8*>(z + (int64_t)b0 * E + i);
    __syncthreads();
    bool own[BMAX];                                          // GROUPED: the clips of this pass that belong to head g
    if constexpr (GROUPED) {
#pragma unroll
      for (int i = 0; i < BMAX; ++i) own[i] = i < nb && group[b0 + i] == g;
    }
    auto mine = [&](int i) { return GROUPED ? own[i] : i < nb; };
    for (int rr = 0; rr < RIDGE_ROWS / 4; ++rr) {
      const int v = vb * RIDGE_ROWS + wave * (RIDGE_ROWS / 4) + rr;
      if (v >= V) break;
      const int64_t row = (int64_t)g * V + v;
      float dp[BMAX];
      float db = 0.f;
#pragma unroll
      for (int i = 0; i < BMAX; ++i) {
        dp[i] = mine(i) ? dpred_own<CORR>(pred, y, b0 + i, v, V, gscale, coef) : 0.f;
        db += dp[i];
      }
      if (lane == 0) dbias[row] = (b0 == 0 ? 0.f : dbias[row]) + db;
      const bf16* wr = W + row * E;
#pragma unroll 4
      for (int c = lane * 8; c < E; c += 512) {
        float gr[8];
        float* o = dW + row * E + c;
        if (b0 == 0) {
          float w[8]; ld8(wr + c, w);
#pragma unroll
          for (int j = 0; j < 8; ++j) gr[j] = l2coef * w[j];
        } else {
          const f32x4 lo = *reinterpret_cast<const f32x4*>(o), hi = *reinterpret_cast<const f32x4*>(o + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { gr[j] = lo[j]; gr[4 + j] = hi[j]; }
        }
#pragma unroll
        for (int i = 0; i < BMAX; ++i) {
          if (mine(i)) {
            float zz[8]; ld8(reinterpret_cast<const bf16*>(zsm) + (int64_t)i * E + c, zz);
#pragma unroll
            for (int j = 0; j < 8; ++j) gr[j] += dp[i] * zz[j];
          }
        }
        *reinterpret_cast<f32x4*>(o) = f32x4{gr[0], gr[1], gr[2], gr[3]};
        *reinterpret_cast<f32x4*>(o + 4) = f32x4{gr[4], gr[5], gr[6], gr[7]};
      }
    }
  }
}
// ---------------------------------------------------------------- backward 2: dz partials over V splits (B > 16)
// grid (ceil(E/512), DZ_SPLIT), block 256 (4 waves share a split's rows); out part[split][B][E].  GROUPED: the split's rows of
// every head are walked in turn, heads ascending; clip b accumulates only over the rows of head group[b], in the plain order.
template <int CORR, bool GROUPED>
__global__ __launch_bounds__(256) void ridge_bwd_z_kernel(const bf16* __restrict__ W, const float* __restrict__ pred,
                                                          const float* __restrict__ y, const int* __restrict__ group,
                                                          float* __restrict__ part, int B, int E, int V, int G, float gscale,
                                                          const float* __restrict__ coef) {
  __shared__ float red[3][BMAX][512];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 512 + lane * 8;
  const int per = (V + DZ_SPLIT - 1) / DZ_SPLIT;
  const int v0 = blockIdx.y * per, v1 = min(V, v0 + per);
  for (int b0 = 0; b0 < B; b0 += BMAX) {
    const int nb = min(BMAX, B - b0);
    int gi[BMAX];                                            // GROUPED: head of every clip of this pass
    if constexpr (GROUPED) {
#pragma unroll
      for (int i = 0; i < BMAX; ++i) gi[i] = i < nb ? group[b0 + i] : -1;
    }
    float acc[BMAX][8];
#pragma unroll
    for (int i = 0; i < BMAX; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[i][j] = 0.f;
    auto walk = [&](int g, auto mine) {                      // this split's rows of head g, for the clips that are mine(i)
      for (int v = v0 + wave; v < v1; v += 4) {
        float w[8]; ld8(W + ((int64_t)g * V + v) * E + c, w);
#pragma unroll
        for (int i = 0; i < BMAX; ++i) {
          if (mine(i)) {
            const float dp = dpred_own<CORR>(pred, y, b0 + i, v, V, gscale, coef);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] += dp * w[j];
          }
        }
      }
    };
    if (c < E) {
      if constexpr (GROUPED) {
        for (int g = 0; g < G; ++g) {
          bool any = false;
#pragma unroll
          for (int i = 0; i < BMAX; ++i) any = any || gi[i] == g;
          if (!any) continue;                                // no clip of this pass reads head g: skip its rows
          walk(g, [&](int i) { return gi[i] == g; });
        }
      } else {
        walk(0, [&](int i) { return i < nb; });
      }
    }
    __syncthreads();
    if (wave > 0) {
#pragma unroll
      for (int i = 0; i < BMAX; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) red[wave - 1][i][lane * 8 + j] = acc[i][j];
    }
    __syncthreads();
    if (wave == 0 && c < E) {
#pragma unroll
      for (int i = 0; i < BMAX; ++i) {
        if (i < nb) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            part[((int64_t)blockIdx.y * B + b0 + i) * E + c + j] =
                acc[i][j] + red[0][i][lane * 8 + j] + red[1][i][lane * 8 + j] + red[2][i][lane * 8 + j];
        }
      }
    }
  }
}
// ---------------------------------------------------------------- backward 3a: sum dz partials, apply dropout
__global__ __launch_bounds__(256) void head_dz_reduce_kernel(const float* __restrict__ part, const float* __restrict__ keep,
                                                             float* __restrict__ dz, int B, int E) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float d = 0.f;
#pragma unroll 8
  for (int k = 0; k < DZ_SPLIT; ++k) d += part[((int64_t)k * B + b) * E + e];
  if (keep) d *= keep[(int64_t)b * E + e];
  dz[(int64_t)b * E + e] = d;
}
__global__ __launch_bounds__(256) void head_dz_from16_kernel(const float* __restrict__ dz16, const float* __restrict__ keep,
                                                             float* __restrict__ dz, int E) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float d = dz16[(int64_t)b * E + e];
  if (keep) d *= keep[(int64_t)b * E + e];
  dz[(int64_t)b * E + e] = d;
}
// ---------------------------------------------------------------- backward 3b: LN2 backward per clip -> dpooled (in place of draw ws)
__global__ __launch_bounds__(1024) void head_ln2_bwd_kernel(const float* __restrict__ dz, const bf16* __restrict__ g2,
                                                            const float* __restrict__ zhat, const float* __restrict__ ln2_rstd,
                                                            float* __restrict__ dpooled, int E) {
  __shared__ float red[16];
  const int b = blockIdx.x;
  float s1 = 0.f, s2 = 0.f;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    const float g = dz[(int64_t)b * E + e] * (float)g2[e];
    s1 += g; s2 += g * zhat[(int64_t)b * E + e];
  }
  const float m1 = block_sum(s1, red) / E;
  const float m2 = block_sum(s2, red) / E;
  const float rstd = ln2_rstd[b];
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    const float g = dz[(int64_t)b * E + e] * (float)g2[e];
    dpooled[(int64_t)b * E + e] = rstd * (g - m1 - zhat[(int64_t)b * E + e] * m2);     // d loss / d pooled[b,e]
  }
}
// ---------------------------------------------------------------- backward 3c: norm-parameter grads (sum over clips), draw
__global__ __launch_bounds__(256) void head_param_grads_kernel(const float* __restrict__ dz, float* __restrict__ dpooled,
                                                               const bf16* __restrict__ g1, const float* __restrict__ pooled_raw,
                                                               const float* __restrict__ sumw, const float* __restrict__ zhat,
                                                               float* __restrict__ dg2, float* __restrict__ db2,
                                                               float* __restrict__ dg1, float* __restrict__ db1, int B, int E) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float a2 = 0.f, c2 = 0.f, a1 = 0.f, c1 = 0.f;
  const float gg = (float)g1[e];
  for (int b = 0; b < B; ++b) {
    const float d = dz[(int64_t)b * E + e], dp = dpooled[(int64_t)b * E + e];
    a2 += d * zhat[(int64_t)b * E + e];
    c2 += d;
    a1 += dp * pooled_raw[(int64_t)b * E + e];
    c1 += dp * sumw[b];
    dpooled[(int64_t)b * E + e] = dp * gg;           // becomes d loss / d pooled_raw[b,e]
  }
  dg2[e] = a2; db2[e] = c2; dg1[e] = a1; db1[e] = c1;
}
// ---------------------------------------------------------------- backward 4: d hidden (one wave per token)
__global__ __launch_bounds__(256) void head_dhidden_kernel(const bf16* __restrict__ hidden, const float* __restrict__ wmask,
                                                           const float* __restrict__ stats, const float* __restrict__ draw,
                                                           bf16* __restrict__ dh, int S, int E, int64_t rows, int B,
                                                           const int* __restrict__ cu) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  int64_t b = row / S, dense = row;             // dense = index into the [B,S] mask / stats
  if (cu) {
    int bb = 0;
    while (bb + 1 < B && row >= cu[bb + 1]) ++bb;
    b = bb; dense = b * S + (row - cu[bb]);
  }
  const float w = wmask[dense];
  bf16* dr = dh + row * E;
  if (w == 0.f) {
    for (int c = lane * 8; c < E; c += 512) *reinterpret_cast<bf16x8*>(dr + c) = bf16x8{};
    return;
  }
  const float mu = stats[dense * 2], rstd = stats[dense * 2 + 1];
  const bf16* xr = hidden + row * E;
  const float* u = draw + b * E;
  float s1 = 0.f, s2 = 0.f;
  for (int c = lane * 8; c < E; c += 512) {
    float x[8]; ld8(xr + c, x);
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float g = w * u[c + j]; s1 += g; s2 += g * (x[j] - mu) * rstd; }
  }
  const float m1 = wave_sum(s1) / E, m2 = wave_sum(s2) / E;
  for (int c = lane * 8; c < E; c += 512) {
    float x[8]; ld8(xr + c, x);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = (bf16)(rstd * (w * u[c + j] - m1 - (x[j] - mu) * rstd * m2));
    *reinterpret_cast<bf16x8*>(dr + c) = o;
  }
}

// ---------------------------------------------------------------- backward 4, accumulate form: dx += d hidden of a lower tap
// head_dhidden_kernel's value added into a dx that already holds the gradient from the layers above: live rows (w != 0) are
// read, added to in fp32 and rounded once; rows with w == 0 are neither read nor written.  One wave per token, one writer
// per element, no atomics.  HBM-bound: a live row of hidden is read ONCE and held in registers (raw bf16, NI = ceil(E/512)
// chunks of 8 columns per lane, all loads in flight together, as head_pool_kernel keeps its row) across the two passes,
// and dx is read while the sums are formed; the additions run in head_dhidden_kernel's order (chunk, then column).
template <int NI>
__global__ __launch_bounds__(256) void head_dhidden_acc_kernel(const bf16* __restrict__ hidden, const float* __restrict__ wmask,
                                                               const float* __restrict__ stats, const float* __restrict__ draw,
                                                               bf16* __restrict__ dh, int S, int E, int64_t rows, int B,
                                                               const int* __restrict__ cu) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= rows) return;
  int64_t b = row / S, dense = row;
  if (cu) {
    int bb = 0;
    while (bb + 1 < B && row >= cu[bb + 1]) ++bb;
    b = bb; dense = b * S + (row - cu[bb]);
  }
  const float w = wmask[dense];
  if (w == 0.f) return;
  bf16* dr = dh + row * E;
  const float mu = stats[dense * 2], rstd = stats[dense * 2 + 1];
  const bf16* xr = hidden + row * E;
  const float* u = draw + b * E;
  bf16x8 xs[NI], ds[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = lane * 8 + i * 512;
    xs[i] = c < E ? *reinterpret_cast<const bf16x8*>(xr + c) : bf16x8{};
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = lane * 8 + i * 512;
    ds[i] = c < E ? *reinterpret_cast<const bf16x8*>(dr + c) : bf16x8{};
  }
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = lane * 8 + i * 512;
    if (c < E) {
#pragma unroll
      for (int j = 0; j < 8; ++j) { const float g = w * u[c + j]; s1 += g; s2 += g * ((float)xs[i][j] - mu) * rstd; }
    }
  }
  const float m1 = wave_sum(s1) / E, m2 = wave_sum(s2) / E;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int c = lane * 8 + i * 512;
    if (c < E) {
      float val[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) val[j] = rstd * (w * u[c + j] - m1 - ((float)xs[i][j] - mu) * rstd * m2);
      bf16x8 o;
      {
#pragma clang fp contract(off)        // the add stays an add: val is the write-mode value, rounded to fp32 as there
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)((float)ds[i][j] + val[j]);
      }
      *reinterpret_cast<bf16x8*>(dr + c) = o;
    }
  }
}

// ---------------------------------------------------------------- layer mix: pooled_raw = sum_k softmax(a)_k P_k
// P_k [B,E] fp32 are the pooled vectors of the K tapped layers (head_reduce_kernel's output per tap); a bf16 [K] the logits'
// compute copy (null: K = 1, alpha = 1).  Every thread recomputes the softmax (K <= 64 exps, no LDS, no second launch) and
// owns 4 consecutive elements; the sum over k runs in ascending order starting FROM the k = 0 term, so K = 1 gives
// 1.0f * P_0 = the bits of P_0 (a signed zero included).  Thread 0 leaves alpha for the backward.
constexpr int MIX_KMAX = 64;
constexpr int MIX_CHUNK = 1024;    // elements per block: 256 threads x f32x4

__device__ __forceinline__ void mix_softmax_stats(const bf16* __restrict__ a, int K, float& amax, float& inv) {
  amax = (float)a[0];
  for (int k = 1; k < K; ++k) amax = fmaxf(amax, (float)a[k]);
  float s = 0.f;
  for (int k = 0; k < K; ++k) s += expf((float)a[k] - amax);
  inv = 1.f / s;
}

__global__ __launch_bounds__(256) void head_mix_fwd_kernel(const float* __restrict__ pstack, const bf16* __restrict__ a,
                                                           float* __restrict__ alpha, float* __restrict__ pooled_raw, int K,
                                                           int64_t n) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  float amax = 0.f, inv = 1.f;
  if (a) mix_softmax_stats(a, K, amax, inv);
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int k = 0; k < K; ++k) alpha[k] = a ? expf((float)a[k] - amax) * inv : 1.f;
  if (i >= n) return;                                  // n is a multiple of 8 (E % 8 == 0)
  auto al_of = [&](int k) { return a ? expf((float)a[k] - amax) * inv : 1.f; };
  const float al0 = al_of(0);
  const f32x4 p0 = *reinterpret_cast<const f32x4*>(pstack + i);
  f32x4 acc = f32x4{al0 * p0[0], al0 * p0[1], al0 * p0[2], al0 * p0[3]};
  for (int k = 1; k < K; ++k) {
    const float al = al_of(k);
    const f32x4 p = *reinterpret_cast<const f32x4*>(pstack + (int64_t)k * n + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += al * p[j];
  }
  *reinterpret_cast<f32x4*>(pooled_raw + i) = acc;
}

// backward 1: block blk owns elements [blk*1024, +1024) of [B,E]: slab[blk][k] = sum over them of draw * P_k (a thread's 4
// products in order, then block_sum: fixed order), and draw_stack[k] = alpha_k * draw on the way (K = 1: alpha = 1.0f, a copy).
__global__ __launch_bounds__(256) void head_mix_bwd_kernel(const float* __restrict__ pstack, const float* __restrict__ draw,
                                                           const float* __restrict__ alpha, float* __restrict__ slab,
                                                           float* __restrict__ draw_stack, int K, int64_t n) {
  __shared__ float red[16];
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  const bool live = i < n;
  const f32x4 d = live ? *reinterpret_cast<const f32x4*>(draw + i) : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < K; ++k) {
    float dot = 0.f;
    if (live) {
      const f32x4 p = *reinterpret_cast<const f32x4*>(pstack + (int64_t)k * n + i);
      const float al = alpha[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) dot += d[j] * p[j];
      *reinterpret_cast<f32x4*>(draw_stack + (int64_t)k * n + i) = f32x4{al * d[0], al * d[1], al * d[2], al * d[3]};
    }
    dot = block_sum(dot, red);
    if (threadIdx.x == 0) slab[(int64_t)blockIdx.x * K + k] = dot;
  }
}

// backward 2, one block of 64: thread k sums its column of the slab in block order, then the softmax Jacobian
//   d a_k = alpha_k (dalpha_k - sum_j alpha_j dalpha_j),  the inner sum in ascending j.  Written, not accumulated.
__global__ __launch_bounds__(64) void head_mix_da_kernel(const float* __restrict__ slab, const float* __restrict__ alpha,
                                                         float* __restrict__ d_a, int K, int nblk) {
  __shared__ float dal[MIX_KMAX];
  const int k = threadIdx.x;
  float s = 0.f;
  if (k < K)
    for (int blk = 0; blk < nblk; ++blk) s += slab[(int64_t)blk * K + k];
  dal[k] = s;
  __syncthreads();
  if (k >= K) return;
  float dot = 0.f;
  for (int j = 0; j < K; ++j) dot += alpha[j] * dal[j];
  d_a[k] = alpha[k] * (s - dot);
}

// ---------------------------------------------------------------- standalone HRFConvolveLayer (src/utils.py:44-56)
// out[b,e] = sum_s w[b,s] * x[b,s,e]: one pass over x, HBM-bound.  grid (HRF_SPLITS, ceil(E/512), B), 4 waves per block; a wave
// walks every 4th token of its split (tokens with zero weight are skipped), a lane owns 8 columns; the four waves are summed
// through LDS and the splits through fp32 slabs in a fixed order (reproducible).  T = bf16 or float embeddings.
constexpr int HRF_SPLITS = 32;

template <typename T>
__global__ __launch_bounds__(256) void hrf_pool_kernel(const T* __restrict__ x, const float* __restrict__ w, float* __restrict__ slab,
                                                       int S, int E) {
  __shared__ float red[3][512];
  const int b = blockIdx.z, c = blockIdx.y * 512 + (threadIdx.x & 63) * 8, wave = threadIdx.x >> 6;
  const int per = (S + HRF_SPLITS - 1) / HRF_SPLITS, s0 = blockIdx.x * per, s1 = min(S, s0 + per);
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (c < E) {
    for (int s = s0 + wave; s < s1; s += 4) {
      const float ws_ = w[(int64_t)b * S + s];
      if (ws_ == 0.f) continue;
      const T* xr = x + ((int64_t)b * S + s) * E + c;
      float v[8];
      if constexpr (sizeof(T) == 2) {
        ld8(reinterpret_cast<const bf16*>(xr), v);
      } else {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(xr), hi = *reinterpret_cast<const f32x4*>(xr + 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) { v[j] = lo[j]; v[4 + j] = hi[j]; }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += ws_ * v[j];
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wave - 1][(threadIdx.x & 63) * 8 + j] = acc[j];
  }
  __syncthreads();
  if (wave == 0 && c < E) {
    float* dst = slab + ((int64_t)b * HRF_SPLITS + blockIdx.x) * E + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = (threadIdx.x & 63) * 8 + j;
      dst[j] = ((acc[j] + red[0][k]) + red[1][k]) + red[2][k];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void hrf_pool_reduce_kernel(const float* __restrict__ slab, T* __restrict__ out, int E) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e >= E) return;
  float a = 0.f;
  for (int k = 0; k < HRF_SPLITS; ++k) a += slab[((int64_t)b * HRF_SPLITS + k) * E + e];
  out[(int64_t)b * E + e] = (T)a;
}

int reserve_ridge_lds(int bytes) {
  static int reserved = 0;
  if (bytes > reserved) {
    // every instantiation that stages z in dynamic LDS
    const void* const kernels[] = {
        reinterpret_cast<const void*>(&ridge_fwd_kernel<false>),          reinterpret_cast<const void*>(&ridge_fwd_kernel<true>),
        reinterpret_cast<const void*>(&ridge_bwd_w_kernel<false, false>), reinterpret_cast<const void*>(&ridge_bwd_w_kernel<false, true>),
        reinterpret_cast<const void*>(&ridge_bwd_w_kernel<true, false>),  reinterpret_cast<const void*>(&ridge_bwd_w_kernel<true, true>)};
    for (const void* k : kernels)
      if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        vlb_set_error("head: cannot reserve %d bytes of LDS for z", bytes);
        return VLB_ERR_LAUNCH;
      }
    reserved = bytes;
  }
  return VLB_OK;
}

template <int NI>
int launch_pool(const bf16* hidden, const float* wmask, float* partial, float* stats, int B, int S, int E, float eps,
                const int* cu, hipStream_t st) {
  const int lds = (4 * E + 8) * sizeof(float);
  // once per process and kernel; a function-local static's initialisation is thread-safe (C++11)
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&head_pool_kernel<NI>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (4 * NI * 512 + 8) * (int)sizeof(float));
  if (attr != hipSuccess) { vlb_set_error("head: LDS reservation failed: %s", hipGetErrorString(attr)); return VLB_ERR_LAUNCH; }
  dim3 grid((S + POOL_ROWS - 1) / POOL_ROWS, B);
  hipLaunchKernelGGL((head_pool_kernel<NI>), grid, dim3(512), lds, st, hidden, wmask, partial, stats, S, E, eps, cu);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// LN1 statistics + weighted pool into per-block slabs (at ws), then their fixed-order sum: the pooling half of the forward.
// vlb_head_fwd and vlb_head_pool both run this, so they give the same (stats, pooled_raw, sumw) bits for the same input.
int head_pool(const void* hidden, const float* wmask, float* partial, float* stats, float* pooled_raw, float* sumw, int B, int S,
              int E, float eps, const int* cu_rows, hipStream_t st) {
  const int nblk = (S + POOL_ROWS - 1) / POOL_ROWS;
  const int ni = (E + 511) / 512;
  int rc;
  if (ni <= 1) rc = launch_pool<1>((const bf16*)hidden, wmask, partial, stats, B, S, E, eps, cu_rows, st);
  else if (ni <= 2) rc = launch_pool<2>((const bf16*)hidden, wmask, partial, stats, B, S, E, eps, cu_rows, st);
  else if (ni <= 4) rc = launch_pool<4>((const bf16*)hidden, wmask, partial, stats, B, S, E, eps, cu_rows, st);
  else if (ni <= 8) rc = launch_pool<8>((const bf16*)hidden, wmask, partial, stats, B, S, E, eps, cu_rows, st);
  else rc = launch_pool<16>((const bf16*)hidden, wmask, partial, stats, B, S, E, eps, cu_rows, st);
  if (rc != VLB_OK) return rc;
  hipLaunchKernelGGL(head_reduce_kernel, dim3((E + 255) / 256, B), dim3(256), 0, st, partial, nblk, pooled_raw, sumw, E);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// floats of ws the backward uses (the dz partials, or the skinny-wgrad slabs + dz16 + d pred^T): the coefficients of the
// correlation objectives (4 per clip) sit right behind, wherever vlb_head_fwd put its own slabs.
int64_t head_bwd_ws_floats(int B, int E, int V) {
  const int64_t dz = (int64_t)DZ_SPLIT * B * E;
  const int64_t dz_mfma = (int64_t)vlb_wgrad_splits(V) * 16 * E + (int64_t)16 * E + ((int64_t)V * 16 + 1) / 2 + 64;
  return dz_mfma > dz ? dz_mfma : dz;
}

// the ridge planner: which forward form, and how many (sum err^2, sum W^2) pairs its launch leaves in lpart - one per block
constexpr int64_t GROUPED_MAX_ROWS = (int64_t)1 << 27;      // G*V: 16 bf16 per row of d pred^T and every tile count fit an int
bool ridge_fwd_is_mfma(int B, int E) { return B <= 16 && E % 128 == 0 && E <= 4096; }
int ridge_fwd_parts(int B, int E, int V, int G, bool mfma) {
  const int64_t ntiles = (int64_t)G * ((V + 15) / 16);      // the MFMA form is persistent over row tiles
  return mfma ? (int)(ntiles < 2048 ? ntiles : 2048) : G * ((V + RIDGE_ROWS - 1) / RIDGE_ROWS);
}

void feature_cache_gather_launch(const float* cache_pooled, const float* cache_sumw, const int* rows, float* pooled_raw,
                                 float* sumw, int B, int E, int n_rows, hipStream_t st) {
  hipLaunchKernelGGL(feature_cache_gather_kernel, dim3((E + 255) / 256, B), dim3(256), 0, st, cache_pooled, cache_sumw, rows,
                     pooled_raw, sumw, E, n_rows);
}

void head_dhidden_launch(const void* hidden, const float* wmask, const float* stats, const float* draw, void* dh, int B, int S,
                         int E, int64_t rows, const int* cu_rows, hipStream_t st) {
  hipLaunchKernelGGL(head_dhidden_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const bf16*)hidden, wmask, stats,
                     draw, (bf16*)dh, S, E, rows, B, cu_rows);
}

// The LN1-affine + LN2 (+ dropout) launch on its own: head_fwd_tail's first launch, and all of vlb_head_features_cached.
int head_ln2_launch(const float* pooled_raw, const float* sumw, const void* ln1_w, const void* ln1_b, const void* ln2_w,
                    const void* ln2_b, const float* keep_scale, float* zhat, float* ln2_rstd, void* z, int B, int E, float eps,
                    hipStream_t st) {
  hipLaunchKernelGGL(head_ln2_kernel, dim3(B), dim3(1024), 0, st, pooled_raw, sumw, (const bf16*)ln1_w, (const bf16*)ln1_b,
                     (const bf16*)ln2_w, (const bf16*)ln2_b, keep_scale, zhat, ln2_rstd, (bf16*)z, E, eps);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// The ridge forward: pred and the loss partials in lpart.  `mfma` = ridge_fwd_is_mfma(B, E) for the head (vlb_ridge_fwd, the
// layer on its own, always runs the scalar form).  -> the number of (sum err^2, sum W^2) pairs written, or an error (< 0).
template <bool GROUPED>
int ridge_fwd_launch_as(const bf16* W, const bf16* bias, const bf16* z, const float* y, const int* group, float* pred,
                        float* lpart, int B, int E, int V, int G, bool mfma, hipStream_t st) {
  const int parts = ridge_fwd_parts(B, E, V, G, mfma);
  if (mfma) {
    const int tpg = (V + 15) / 16, ntiles = G * tpg;
    switch (E / 128) {
#define VLB_RIDGE_CASE(KS) case KS: hipLaunchKernelGGL((ridge_fwd_mfma_kernel<KS, GROUPED>), dim3(parts), dim3(256), 0, st, W, bias, z, \
                                                       y, group, pred, lpart, B, E, V, tpg, ntiles); break;
      VLB_RIDGE_CASE(1) VLB_RIDGE_CASE(2) VLB_RIDGE_CASE(3) VLB_RIDGE_CASE(4) VLB_RIDGE_CASE(5) VLB_RIDGE_CASE(6) VLB_RIDGE_CASE(7)
      VLB_RIDGE_CASE(8) VLB_RIDGE_CASE(9) VLB_RIDGE_CASE(10) VLB_RIDGE_CASE(11) VLB_RIDGE_CASE(12) VLB_RIDGE_CASE(13)
      VLB_RIDGE_CASE(14) VLB_RIDGE_CASE(15) VLB_RIDGE_CASE(16) VLB_RIDGE_CASE(17) VLB_RIDGE_CASE(18) VLB_RIDGE_CASE(19)
      VLB_RIDGE_CASE(20) VLB_RIDGE_CASE(21) VLB_RIDGE_CASE(22) VLB_RIDGE_CASE(23) VLB_RIDGE_CASE(24) VLB_RIDGE_CASE(25)
      VLB_RIDGE_CASE(26) VLB_RIDGE_CASE(27) VLB_RIDGE_CASE(28) VLB_RIDGE_CASE(29) VLB_RIDGE_CASE(30) VLB_RIDGE_CASE(31)
      VLB_RIDGE_CASE(32)
#undef VLB_RIDGE_CASE
    }
  } else {
    const int bpg = (V + RIDGE_ROWS - 1) / RIDGE_ROWS;
    const int zlds = (B < BMAX ? B : BMAX) * E * 2;
    if (int rc = reserve_ridge_lds(zlds)) return rc;
    hipLaunchKernelGGL(ridge_fwd_kernel<GROUPED>, dim3(parts), dim3(256), zlds, st, W, bias, z, y, group, pred, lpart, B, E, V, bpg);
  }
  VLB_LAUNCH_CHECK();
  return parts;
}
int ridge_fwd_launch(const void* W, const void* bias, const void* z, const float* y, const int* group, float* pred, float* lpart,
                     int B, int E, int V, int G, bool mfma, hipStream_t st) {
  return group ? ridge_fwd_launch_as<true>((const bf16*)W, (const bf16*)bias, (const bf16*)z, y, group, pred, lpart, B, E, V, G, mfma, st)
               : ridge_fwd_launch_as<false>((const bf16*)W, (const bf16*)bias, (const bf16*)z, y, nullptr, pred, lpart, B, E, V, 1, mfma, st);
}

// The correlation objectives' forward on a finished pred: row statistics, then the loss terms from them and the ridge partials.
int head_loss_corr_launch(const float* pred, const float* y, const float* lpart, int parts, float* rowstat, float* loss_terms,
                          float* loss_aux, int B, int V, int loss_kind, float l2_lambda, hipStream_t st) {
  if (loss_kind == VLB_LOSS_PEARSON) hipLaunchKernelGGL(head_rowstat_kernel<true>, dim3(B), dim3(1024), 0, st, pred, y, rowstat, V);
  else hipLaunchKernelGGL(head_rowstat_kernel<false>, dim3(B), dim3(1024), 0, st, pred, y, rowstat, V);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(loss_finalize_corr_kernel, dim3(1), dim3(256), 0, st, lpart, parts, 1.f / ((float)B * (float)V), l2_lambda,
                     rowstat, B, loss_terms, loss_aux);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// LN1 affine + LN2 + dropout -> z, ridge GEMV, loss: everything of the forward that reads only (pooled_raw, sumw).
// vlb_head_fwd, vlb_head_fwd_cached (group = nullptr, G = 1) and vlb_head_fwd_grouped all end here, so they give the same bits
// for the same (pooled_raw, sumw).  loss_kind: the plain entries pass VLB_LOSS_MSE (vlb_head_loss_fwd finishes a correlation
// objective in a call of its own); the grouped entry finishes it here.
int head_fwd_tail(const float* pooled_raw, const float* sumw, const void* ln1_w, const void* ln1_b, const void* ln2_w,
                  const void* ln2_b, const void* ridge_w, const void* ridge_b, const float* y, const float* keep_scale,
                  const int* group, float* lpart, float* zhat, float* ln2_rstd, void* z, float* pred, float* rowstat,
                  float* loss_terms, float* loss_aux, int B, int E, int V, int G, float eps, float l2_lambda, int loss_kind,
                  hipStream_t st) {
  if (int rc = head_ln2_launch(pooled_raw, sumw, ln1_w, ln1_b, ln2_w, ln2_b, keep_scale, zhat, ln2_rstd, z, B, E, eps, st)) return rc;
  const int parts = ridge_fwd_launch(ridge_w, ridge_b, z, y, group, pred, lpart, B, E, V, G, ridge_fwd_is_mfma(B, E), st);
  if (parts < 0) return parts;
  if (loss_kind != VLB_LOSS_MSE)
    return head_loss_corr_launch(pred, y, lpart, parts, rowstat, loss_terms, loss_aux, B, V, loss_kind, l2_lambda, st);
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, lpart, parts, 1.f / ((float)B * (float)V), l2_lambda,
                     loss_terms);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// dW, dbias and the unmasked dz of the ridge layer over GV = G*V rows, one (objective, GROUPED) instantiation per call
template <int CORR, bool GROUPED>
int ridge_bwd_launch(const void* ridge_w, const void* z, const float* pred, const float* y, const float* keep_scale,
                     const int* group, float* d_ridge_w, float* d_ridge_b, float* ws, float* dz_ws, const float* coef, int B, int E,
                     int V, int G, float gscale, float l2coef, void* stream) {
  hipStream_t st = as_stream(stream);
  const int GV = G * V;
  const int bpg = (V + RIDGE_ROWS - 1) / RIDGE_ROWS;
  const int zlds = (B < BMAX ? B : BMAX) * E * 2;
  if (int rc2 = reserve_ridge_lds(zlds)) return rc2;
  hipLaunchKernelGGL((ridge_bwd_w_kernel<CORR, GROUPED>), dim3(G * bpg), dim3(256), zlds, st, (const bf16*)ridge_w, (const bf16*)z, pred,
                     y, group, d_ridge_w, d_ridge_b, B, E, V, bpg, gscale, l2coef, coef);
  VLB_LAUNCH_CHECK();
  if (B <= 16 && E % 8 == 0) {
    // dz[b,e] = sum_{(g,v)} dpT[g*V+v, b] W[g*V+v, e]: contraction over the ROWS of W -> ONE MFMA skinny-wgrad call over all
    // G*V rows (G operand = dpred^T [GV,16] bf16, zeros off the clip's head; X = W).  Rows b < B of a [16,E] fp32 block -> dz16.
    const int splits = vlb_wgrad_splits(GV);
    float* wg_ws = ws;                                             // [splits][16][E]
    float* dz16 = ws + (int64_t)splits * 16 * E;                   // [16][E]
    bf16* dpT = reinterpret_cast<bf16*>(dz16 + (int64_t)16 * E);   // [G*V][16] bf16
    hipLaunchKernelGGL((dpred_t_kernel<CORR, GROUPED>), dim3((unsigned)(((int64_t)GV * 16 + 255) / 256)), dim3(256), 0, st, pred, y,
                       group, dpT, B, V, (int64_t)GV, gscale, coef);
    VLB_LAUNCH_CHECK();
    int rc3 = vlb_wgrad_skinny(dpT, 16, ridge_w, E, dz16, wg_ws, GV, 16, E, 1.f, 0.f, 0.f, nullptr, stream);
    if (rc3 != VLB_OK) return rc3;
    hipLaunchKernelGGL(head_dz_from16_kernel, dim3((E + 255) / 256, B), dim3(256), 0, st, dz16, keep_scale, dz_ws, E);
  } else {
    hipLaunchKernelGGL((ridge_bwd_z_kernel<CORR, GROUPED>), dim3((E + 511) / 512, DZ_SPLIT), dim3(256), 0, st, (const bf16*)ridge_w,
                       pred, y, group, ws, B, E, V, G, gscale, coef);
    VLB_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_dz_reduce_kernel, dim3((E + 255) / 256, B), dim3(256), 0, st, ws, keep_scale, dz_ws, B, E);
  }
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// Ridge, dropout, LN2 and LN1-affine gradients (dpooled_ws = d loss / d pooled_raw is left for head_dhidden_kernel): every
// backward entry runs this (the plain ones with group = nullptr, G = 1), so their parameter gradients are the same bits.
// loss_kind = LOSS_FROM_DPRED (vlb_head_bwd_wloss): `pred` is the finished d pred [B,V]; y, rowstat and loss_scale are not used.
constexpr int LOSS_FROM_DPRED = -1;
int head_bwd_params(const void* ln1_w, const void* ln2_w, const void* ridge_w, const float* y, const float* keep_scale,
                    const int* group, const float* pooled_raw, const float* sumw, const float* zhat, const float* ln2_rstd,
                    const void* z, const float* pred, float* d_ridge_w, float* d_ridge_b, float* d_ln2_w, float* d_ln2_b,
                    float* d_ln1_w, float* d_ln1_b, float* ws, float* dz_ws, float* dpooled_ws, const float* rowstat, int B, int E,
                    int V, int G, float l2_lambda, float loss_scale, float l2_scale, int loss_kind, void* stream) {
  hipStream_t st = as_stream(stream);
  const float gscale = loss_scale * 2.f / ((float)B * (float)V);      // B: the whole batch, whatever the heads' shares
  const float l2coef = l2_scale * 2.f * l2_lambda;
  // correlation objectives: the per-clip coefficients live behind everything the backward keeps in ws
  float* coef = ws + head_bwd_ws_floats(B, E, G * V);
  const bool buf = loss_kind == LOSS_FROM_DPRED, corr = !buf && loss_kind != VLB_LOSS_MSE;
  if (corr) {
    hipLaunchKernelGGL(head_loss_coef_kernel, dim3((B + 63) / 64), dim3(64), 0, st, rowstat, coef, B, loss_scale);
    VLB_LAUNCH_CHECK();
  }
  const auto ridge_bwd = buf    ? (group ? &ridge_bwd_launch<DP_BUF, true> : &ridge_bwd_launch<DP_BUF, false>)
                         : corr ? (group ? &ridge_bwd_launch<DP_CORR, true> : &ridge_bwd_launch<DP_CORR, false>)
                                : (group ? &ridge_bwd_launch<DP_MSE, true> : &ridge_bwd_launch<DP_MSE, false>);
  if (int rc = ridge_bwd(ridge_w, z, pred, y, keep_scale, group, d_ridge_w, d_ridge_b, ws, dz_ws, coef, B, E, V, G, gscale, l2coef,
                         stream))
    return rc;
  hipLaunchKernelGGL(head_ln2_bwd_kernel, dim3(B), dim3(1024), 0, st, dz_ws, (const bf16*)ln2_w, zhat, ln2_rstd, dpooled_ws, E);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_param_grads_kernel, dim3((E + 255) / 256), dim3(256), 0, st, dz_ws, dpooled_ws, (const bf16*)ln1_w,
                     pooled_raw, sumw, zhat, d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, B, E);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}
}  // namespace

extern "C" int vlb_head_partial_rows(int S) { return (S + POOL_ROWS - 1) / POOL_ROWS; }
extern "C" int64_t vlb_head_ws_floats(int B, int S, int E, int V) {
  const int64_t pool = (int64_t)B * vlb_head_partial_rows(S) * (E + 2);
  const int64_t ridge = 2 * (int64_t)((V + RIDGE_ROWS - 1) / RIDGE_ROWS);
  const int64_t bwd = head_bwd_ws_floats(B, E, V) + 4 * (int64_t)B;      // + coef[B][4] of the correlation objectives
  const int64_t m = pool + ridge;
  return bwd > m ? bwd : m;
}

extern "C" int vlb_head_fwd(const void* hidden, const float* wmask, const void* ln1_w, const void* ln1_b,
                            const void* ln2_w, const void* ln2_b, const void* ridge_w, const void* ridge_b,
                            const float* y, const float* keep_scale, float* ws, float* stats, float* pooled_raw,
                            float* sumw, float* zhat, float* ln2_rstd, void* z, float* pred, float* loss_terms, int B,
                            int S, int E, int V, float eps, float l2_lambda, const int* cu_rows, void* stream) {
  VLB_REQUIRE(hidden && wmask && ln1_w && ln1_b && ln2_w && ln2_b && ridge_w && ridge_b && y && ws && stats &&
                  pooled_raw && sumw && zhat && ln2_rstd && z && pred && loss_terms, "head_fwd: null argument");
  VLB_REQUIRE(B > 0 && S > 0 && V > 0 && E % 8 == 0 && E > 0 && E <= 8192, "head_fwd: bad shape B=%d S=%d E=%d V=%d", B, S, E, V);
  hipStream_t st = as_stream(stream);
  float* lpart = ws + (int64_t)B * vlb_head_partial_rows(S) * (E + 2);
  if (int rc = head_pool(hidden, wmask, ws, stats, pooled_raw, sumw, B, S, E, eps, cu_rows, st)) return rc;
  return head_fwd_tail(pooled_raw, sumw, ln1_w, ln1_b, ln2_w, ln2_b, ridge_w, ridge_b, y, keep_scale, nullptr, lpart, zhat,
                       ln2_rstd, z, pred, nullptr, loss_terms, nullptr, B, E, V, 1, eps, l2_lambda, VLB_LOSS_MSE, st);
}

namespace {
// vlb_head_bwd (loss_kind = VLB_LOSS_MSE, rowstat = nullptr) and vlb_head_bwd_loss, which checks its loss_kind first
int head_bwd_entry(const char* who, const void* hidden, const float* wmask, const void* ln1_w, const void* ln2_w,
                   const void* ridge_w, const float* y, const float* keep_scale, const float* stats, const float* pooled_raw,
                   const float* sumw, const float* zhat, const float* ln2_rstd, const void* z, const float* pred,
                   float* d_ridge_w, float* d_ridge_b, float* d_ln2_w, float* d_ln2_b, float* d_ln1_w, float* d_ln1_b, float* ws,
                   float* dz_ws, float* dpooled_ws, void* dhidden, int B, int S, int E, int V, float l2_lambda, float loss_scale,
                   float l2_scale, const int* cu_rows, int total_rows, void* stream, int loss_kind, const float* rowstat) {
  VLB_REQUIRE(hidden && wmask && ln1_w && ln2_w && ridge_w && y && stats && pooled_raw && sumw && zhat && ln2_rstd && z &&
                  pred && d_ridge_w && d_ridge_b && d_ln2_w && d_ln2_b && d_ln1_w && d_ln1_b && ws && dz_ws && dpooled_ws,
              "%s: null argument", who);
  VLB_REQUIRE(B > 0 && S > 0 && V > 0 && E % 8 == 0 && E > 0 && E <= 8192, "%s: bad shape", who);
  const int64_t rows = cu_rows ? (int64_t)total_rows : (int64_t)B * S;
  VLB_REQUIRE(!dhidden || (rows > 0 && rows <= (int64_t)B * S), "%s: total_rows=%d out of range", who, total_rows);
  if (int rc = head_bwd_params(ln1_w, ln2_w, ridge_w, y, keep_scale, nullptr, pooled_raw, sumw, zhat, ln2_rstd, z, pred, d_ridge_w,
                               d_ridge_b, d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, ws, dz_ws, dpooled_ws, rowstat, B, E, V, 1, l2_lambda,
                               loss_scale, l2_scale, loss_kind, stream))
    return rc;
  if (dhidden) {
    head_dhidden_launch(hidden, wmask, stats, dpooled_ws, dhidden, B, S, E, rows, cu_rows, as_stream(stream));
    VLB_LAUNCH_CHECK();
  }
  return VLB_OK;
}

// vlb_head_bwd_cached and vlb_head_bwd_cached_loss likewise
int head_bwd_cached_entry(const char* who, const void* ln1_w, const void* ln2_w, const void* ridge_w, const float* y,
                          const float* keep_scale, const float* pooled_raw, const float* sumw, const float* zhat,
                          const float* ln2_rstd, const void* z, const float* pred, float* d_ridge_w, float* d_ridge_b,
                          float* d_ln2_w, float* d_ln2_b, float* d_ln1_w, float* d_ln1_b, float* ws, float* dz_ws, float* dpooled_ws,
                          int B, int E, int V, float l2_lambda, float loss_scale, float l2_scale, void* stream, int loss_kind,
                          const float* rowstat) {
  VLB_REQUIRE(ln1_w && ln2_w && ridge_w && y && pooled_raw && sumw && zhat && ln2_rstd && z && pred && d_ridge_w && d_ridge_b &&
                  d_ln2_w && d_ln2_b && d_ln1_w && d_ln1_b && ws && dz_ws && dpooled_ws,
              "%s: null argument", who);
  VLB_REQUIRE(B > 0 && V > 0 && E % 8 == 0 && E > 0 && E <= 8192, "%s: bad shape", who);
  return head_bwd_params(ln1_w, ln2_w, ridge_w, y, keep_scale, nullptr, pooled_raw, sumw, zhat, ln2_rstd, z, pred, d_ridge_w,
                         d_ridge_b, d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, ws, dz_ws, dpooled_ws, rowstat, B, E, V, 1, l2_lambda,
                         loss_scale, l2_scale, loss_kind, stream);
}
}  // namespace

extern "C" int vlb_head_bwd(const void* hidden, const float* wmask, const void* ln1_w, const void* ln2_w,
                            const void* ridge_w, const float* y, const float* keep_scale, const float* stats,
                            const float* pooled_raw, const float* sumw, const float* zhat, const float* ln2_rstd,
                            const void* z, const float* pred, float* d_ridge_w, float* d_ridge_b, float* d_ln2_w,
                            float* d_ln2_b, float* d_ln1_w, float* d_ln1_b, float* ws, float* dz_ws, float* dpooled_ws,
                            void* dhidden, int B, int S, int E, int V, float eps, float l2_lambda, float loss_scale,
                            float l2_scale, const int* cu_rows, int total_rows, void* stream) {
  (void)eps;
  return head_bwd_entry("head_bwd", hidden, wmask, ln1_w, ln2_w, ridge_w, y, keep_scale, stats, pooled_raw, sumw, zhat, ln2_rstd, z,
                        pred, d_ridge_w, d_ridge_b, d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, ws, dz_ws, dpooled_ws, dhidden, B, S, E, V,
                        l2_lambda, loss_scale, l2_scale, cu_rows, total_rows, stream, VLB_LOSS_MSE, nullptr);
}

// ---------------------------------------------------------------- frozen-backbone feature cache
extern "C" int vlb_feature_cache_store(const float* pooled_raw, const float* sumw, const int* rows, float* cache_pooled,
                                       float* cache_sumw, int B, int E, int n_rows, void* stream) {
  VLB_REQUIRE(pooled_raw && sumw && rows && cache_pooled && cache_sumw, "feature_cache_store: null argument");
  VLB_REQUIRE(B > 0 && E > 0 && n_rows > 0, "feature_cache_store: bad shape B=%d E=%d n_rows=%d", B, E, n_rows);
  hipLaunchKernelGGL(feature_cache_store_kernel, dim3((E + 255) / 256, B), dim3(256), 0, as_stream(stream), pooled_raw, sumw,
                     rows, cache_pooled, cache_sumw, E, n_rows);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_head_fwd_cached(const float* cache_pooled, const float* cache_sumw, const int* rows, const void* ln1_w,
                                   const void* ln1_b, const void* ln2_w, const void* ln2_b, const void* ridge_w,
                                   const void* ridge_b, const float* y, const float* keep_scale, float* ws, float* pooled_raw,
                                   float* sumw, float* zhat, float* ln2_rstd, void* z, float* pred, float* loss_terms, int B,
                                   int E, int V, int n_rows, float eps, float l2_lambda, void* stream) {
  VLB_REQUIRE(cache_pooled && cache_sumw && rows && ln1_w && ln1_b && ln2_w && ln2_b && ridge_w && ridge_b && y && ws &&
                  pooled_raw && sumw && zhat && ln2_rstd && z && pred && loss_terms, "head_fwd_cached: null argument");
  VLB_REQUIRE(B > 0 && V > 0 && n_rows > 0 && E % 8 == 0 && E > 0 && E <= 8192,
              "head_fwd_cached: bad shape B=%d E=%d V=%d n_rows=%d", B, E, V, n_rows);
  hipStream_t st = as_stream(stream);
  feature_cache_gather_launch(cache_pooled, cache_sumw, rows, pooled_raw, sumw, B, E, n_rows, st);
  VLB_LAUNCH_CHECK();
  return head_fwd_tail(pooled_raw, sumw, ln1_w, ln1_b, ln2_w, ln2_b, ridge_w, ridge_b, y, keep_scale, nullptr, ws, zhat, ln2_rstd, z,
                       pred, nullptr, loss_terms, nullptr, B, E, V, 1, eps, l2_lambda, VLB_LOSS_MSE, st);
}

// The features the ridge layer reads, for the closed-form fit (ridge_solve.hip): the same gather, the same LN2 launch with
// keep_scale = NULL, and nothing after it - no ridge, no loss.
extern "C" int vlb_head_features_cached(const float* cache_pooled, const float* cache_sumw, const int* rows, const void* ln1_w,
                                        const void* ln1_b, const void* ln2_w, const void* ln2_b, float* pooled_raw, float* sumw,
                                        float* zhat, float* ln2_rstd, void* z, int B, int E, int n_rows, float eps, void* stream) {
  VLB_REQUIRE(cache_pooled && cache_sumw && rows && ln1_w && ln1_b && ln2_w && ln2_b && pooled_raw && sumw && zhat && ln2_rstd && z,
              "head_features_cached: null argument");
  VLB_REQUIRE(B > 0 && n_rows > 0 && E % 8 == 0 && E > 0 && E <= 8192, "head_features_cached: bad shape B=%d E=%d n_rows=%d", B, E,
              n_rows);
  hipStream_t st = as_stream(stream);
  feature_cache_gather_launch(cache_pooled, cache_sumw, rows, pooled_raw, sumw, B, E, n_rows, st);
  VLB_LAUNCH_CHECK();
  return head_ln2_launch(pooled_raw, sumw, ln1_w, ln1_b, ln2_w, ln2_b, nullptr, zhat, ln2_rstd, z, B, E, eps, st);
}

extern "C" int vlb_head_bwd_cached(const void* ln1_w, const void* ln2_w, const void* ridge_w, const float* y,
                                   const float* keep_scale, const float* pooled_raw, const float* sumw, const float* zhat,
                                   const float* ln2_rstd, const void* z, const float* pred, float* d_ridge_w, float* d_ridge_b,
                                   float* d_ln2_w, float* d_ln2_b, float* d_ln1_w, float* d_ln1_b, float* ws, float* dz_ws,
                                   float* dpooled_ws, int B, int E, int V, float eps, float l2_lambda, float loss_scale,
                                   float l2_scale, void* stream) {
  (void)eps;
  return head_bwd_cached_entry("head_bwd_cached", ln1_w, ln2_w, ridge_w, y, keep_scale, pooled_raw, sumw, zhat, ln2_rstd, z, pred,
                               d_ridge_w, d_ridge_b, d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, ws, dz_ws, dpooled_ws, B, E, V, l2_lambda,
                               loss_scale, l2_scale, stream, VLB_LOSS_MSE, nullptr);
}

// ---------------------------------------------------------------- correlation objectives: entry points
extern "C" int vlb_head_loss_fwd(const float* pred, const float* y, const float* ws, float* rowstat, float* loss_terms,
                                 float* loss_aux, int B, int S, int E, int V, int loss_kind, float l2_lambda, void* stream) {
  VLB_REQUIRE(pred && y && ws && rowstat && loss_terms && loss_aux, "head_loss_fwd: null argument");
  VLB_REQUIRE(loss_kind != VLB_LOSS_MSE, "head_loss_fwd: loss_kind 0 (mse) is what vlb_head_fwd itself computes");
  VLB_REQUIRE(loss_kind == VLB_LOSS_COSINE || loss_kind == VLB_LOSS_PEARSON, "head_loss_fwd: unknown loss_kind %d", loss_kind);
  VLB_REQUIRE(B > 0 && S >= 0 && V > 0 && E % 8 == 0 && E > 0 && E <= 8192, "head_loss_fwd: bad shape B=%d S=%d E=%d V=%d", B, S, E, V);
  VLB_REQUIRE(loss_kind != VLB_LOSS_PEARSON || V >= 2, "head_loss_fwd: pearson needs V >= 2 (V=%d)", V);
  // where the forward left the ridge partials: behind the pooling slabs (vlb_head_fwd), or at ws (vlb_head_fwd_cached)
  const float* lpart = ws + (S > 0 ? (int64_t)B * vlb_head_partial_rows(S) * (E + 2) : 0);
  return head_loss_corr_launch(pred, y, lpart, ridge_fwd_parts(B, E, V, 1, ridge_fwd_is_mfma(B, E)), rowstat, loss_terms, loss_aux, B,
                               V, loss_kind, l2_lambda, as_stream(stream));
}

extern "C" int vlb_head_bwd_loss(const void* hidden, const float* wmask, const void* ln1_w, const void* ln2_w,
                                 const void* ridge_w, const float* y, const float* keep_scale, const float* stats,
                                 const float* pooled_raw, const float* sumw, const float* zhat, const float* ln2_rstd,
                                 const void* z, const float* pred, float* d_ridge_w, float* d_ridge_b, float* d_ln2_w,
                                 float* d_ln2_b, float* d_ln1_w, float* d_ln1_b, float* ws, float* dz_ws, float* dpooled_ws,
                                 void* dhidden, int B, int S, int E, int V, float eps, float l2_lambda, float loss_scale,
                                 float l2_scale, const int* cu_rows, int total_rows, void* stream, int loss_kind,
                                 const float* rowstat) {
  (void)eps;
  VLB_REQUIRE(rowstat, "head_bwd_loss: null argument");
  VLB_REQUIRE(loss_kind != VLB_LOSS_MSE, "head_bwd_loss: loss_kind 0 (mse) is vlb_head_bwd's");
  VLB_REQUIRE(loss_kind == VLB_LOSS_COSINE || loss_kind == VLB_LOSS_PEARSON, "head_bwd_loss: unknown loss_kind %d", loss_kind);
  VLB_REQUIRE(loss_kind != VLB_LOSS_PEARSON || V >= 2, "head_bwd_loss: pearson needs V >= 2 (V=%d)", V);
  return head_bwd_entry("head_bwd_loss", hidden, wmask, ln1_w, ln2_w, ridge_w, y, keep_scale, stats, pooled_raw, sumw, zhat, ln2_rstd,
                        z, pred, d_ridge_w, d_ridge_b, d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, ws, dz_ws, dpooled_ws, dhidden, B, S, E, V,
                        l2_lambda, loss_scale, l2_scale, cu_rows, total_rows, stream, loss_kind, rowstat);
}

extern "C" int vlb_head_bwd_cached_loss(const void* ln1_w, const void* ln2_w, const void* ridge_w, const float* y,
                                        const float* keep_scale, const float* pooled_raw, const float* sumw, const float* zhat,
                                        const float* ln2_rstd, const void* z, const float* pred, float* d_ridge_w,
                                        float* d_ridge_b, float* d_ln2_w, float* d_ln2_b, float* d_ln1_w, float* d_ln1_b, float* ws,
                                        float* dz_ws, float* dpooled_ws, int B, int E, int V, float eps, float l2_lambda,
                                        float loss_scale, float l2_scale, void* stream, int loss_kind, const float* rowstat) {
  (void)eps;
  VLB_REQUIRE(rowstat, "head_bwd_cached_loss: null argument");
  VLB_REQUIRE(loss_kind != VLB_LOSS_MSE, "head_bwd_cached_loss: loss_kind 0 (mse) is vlb_head_bwd_cached's");
  VLB_REQUIRE(loss_kind == VLB_LOSS_COSINE || loss_kind == VLB_LOSS_PEARSON, "head_bwd_cached_loss: unknown loss_kind %d", loss_kind);
  VLB_REQUIRE(loss_kind != VLB_LOSS_PEARSON || V >= 2, "head_bwd_cached_loss: pearson needs V >= 2 (V=%d)", V);
  return head_bwd_cached_entry("head_bwd_cached_loss", ln1_w, ln2_w, ridge_w, y, keep_scale, pooled_raw, sumw, zhat, ln2_rstd, z, pred,
                               d_ridge_w, d_ridge_b, d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, ws, dz_ws, dpooled_ws, B, E, V, l2_lambda,
                               loss_scale, l2_scale, stream, loss_kind, rowstat);
}

// ---------------------------------------------------------------- per-subject ridge heads on one trunk: the grouped tail
extern "C" int64_t vlb_head_grouped_ws_floats(int B, int E, int V, int G) {
  if (B <= 0 || E <= 0 || V <= 0 || G <= 0 || (int64_t)G * V > GROUPED_MAX_ROWS) return 0;
  const int64_t fwd = 2 * (int64_t)G * ((V + 15) / 16);                  // >= 2 * ridge_fwd_parts, either form
  const int64_t bwd = head_bwd_ws_floats(B, E, G * V) + 4 * (int64_t)B;  // + coef[B][4] of the correlation objectives
  return bwd > fwd ? bwd : fwd;
}

extern "C" int vlb_head_fwd_grouped(const float* cache_pooled, const float* cache_sumw, const int* rows, const void* ln1_w,
                                    const void* ln1_b, const void* ln2_w, const void* ln2_b, const void* ridge_w,
                                    const void* ridge_b, const float* y, const float* keep_scale, const int* group, float* ws,
                                    float* pooled_raw, float* sumw, float* zhat, float* ln2_rstd, void* z, float* pred,
                                    float* rowstat, float* loss_terms, float* loss_aux, int B, int E, int V, int G, int n_rows,
                                    float eps, float l2_lambda, int loss_kind, void* stream) {
  VLB_REQUIRE(cache_pooled && cache_sumw && rows && ln1_w && ln1_b && ln2_w && ln2_b && ridge_w && ridge_b && y && group && ws &&
                  pooled_raw && sumw && zhat && ln2_rstd && z && pred && loss_terms, "head_fwd_grouped: null argument");
  VLB_REQUIRE(loss_kind == VLB_LOSS_MSE || loss_kind == VLB_LOSS_COSINE || loss_kind == VLB_LOSS_PEARSON,
              "head_fwd_grouped: unknown loss_kind %d", loss_kind);
  VLB_REQUIRE(loss_kind == VLB_LOSS_MSE || (rowstat && loss_aux), "head_fwd_grouped: loss_kind %d needs rowstat and loss_aux", loss_kind);
  VLB_REQUIRE(B > 0 && V > 0 && G >= 1 && n_rows > 0 && E % 8 == 0 && E > 0 && E <= 8192,
              "head_fwd_grouped: bad shape B=%d E=%d V=%d G=%d n_rows=%d", B, E, V, G, n_rows);
  VLB_REQUIRE((int64_t)G * V <= GROUPED_MAX_ROWS, "head_fwd_grouped: G*V = %lld rows, at most 2^27", (long long)G * V);
  VLB_REQUIRE(loss_kind != VLB_LOSS_PEARSON || V >= 2, "head_fwd_grouped: pearson needs V >= 2 (V=%d)", V);
  hipStream_t st = as_stream(stream);
  feature_cache_gather_launch(cache_pooled, cache_sumw, rows, pooled_raw, sumw, B, E, n_rows, st);
  VLB_LAUNCH_CHECK();
  return head_fwd_tail(pooled_raw, sumw, ln1_w, ln1_b, ln2_w, ln2_b, ridge_w, ridge_b, y, keep_scale, group, ws, zhat, ln2_rstd, z,
                       pred, rowstat, loss_terms, loss_aux, B, E, V, G, eps, l2_lambda, loss_kind, st);
}

extern "C" int vlb_head_bwd_grouped(const void* ln1_w, const void* ln2_w, const void* ridge_w, const float* y,
                                    const float* keep_scale, const int* group, const float* pooled_raw, const float* sumw,
                                    const float* zhat, const float* ln2_rstd, const void* z, const float* pred, float* d_ridge_w,
                                    float* d_ridge_b, float* d_ln2_w, float* d_ln2_b, float* d_ln1_w, float* d_ln1_b, float* ws,
                                    float* dz_ws, float* dpooled_ws, const float* rowstat, int B, int E, int V, int G, float eps,
                                    float l2_lambda, float loss_scale, float l2_scale, int loss_kind, void* stream) {
  (void)eps;
  VLB_REQUIRE(ln1_w && ln2_w && ridge_w && y && group && pooled_raw && sumw && zhat && ln2_rstd && z && pred && d_ridge_w &&
                  d_ridge_b && d_ln2_w && d_ln2_b && d_ln1_w && d_ln1_b && ws && dz_ws && dpooled_ws,
              "head_bwd_grouped: null argument");
  VLB_REQUIRE(loss_kind == VLB_LOSS_MSE || loss_kind == VLB_LOSS_COSINE || loss_kind == VLB_LOSS_PEARSON,
              "head_bwd_grouped: unknown loss_kind %d", loss_kind);
  VLB_REQUIRE(loss_kind == VLB_LOSS_MSE || rowstat, "head_bwd_grouped: loss_kind %d needs rowstat", loss_kind);
  VLB_REQUIRE(B > 0 && V > 0 && G >= 1 && E % 8 == 0 && E > 0 && E <= 8192, "head_bwd_grouped: bad shape B=%d E=%d V=%d G=%d", B, E, V, G);
  VLB_REQUIRE((int64_t)G * V <= GROUPED_MAX_ROWS, "head_bwd_grouped: G*V = %lld rows, at most 2^27", (long long)G * V);
  VLB_REQUIRE(loss_kind != VLB_LOSS_PEARSON || V >= 2, "head_bwd_grouped: pearson needs V >= 2 (V=%d)", V);
  return head_bwd_params(ln1_w, ln2_w, ridge_w, y, keep_scale, group, pooled_raw, sumw, zhat, ln2_rstd, z, pred, d_ridge_w, d_ridge_b,
                         d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, ws, dz_ws, dpooled_ws, rowstat, B, E, V, G, l2_lambda, loss_scale,
                         l2_scale, loss_kind, stream);
}

// ---------------------------------------------------------------- readout from chosen layers: pool, mix, d hidden on their own
extern "C" int vlb_head_pool(const void* hidden, const float* wmask, float* ws, float* stats, float* pooled_raw, float* sumw, int B,
                             int S, int E, float eps, const int* cu_rows, void* stream) {
  VLB_REQUIRE(hidden && wmask && ws && stats && pooled_raw && sumw, "head_pool: null argument");
  VLB_REQUIRE(B > 0 && S > 0 && E % 8 == 0 && E > 0 && E <= 8192, "head_pool: bad shape B=%d S=%d E=%d", B, S, E);
  return head_pool(hidden, wmask, ws, stats, pooled_raw, sumw, B, S, E, eps, cu_rows, as_stream(stream));
}

extern "C" int vlb_feature_cache_gather(const float* cache_pooled, const float* cache_sumw, const int* rows, float* pooled_raw,
                                        float* sumw, int B, int E, int n_rows, void* stream) {
  VLB_REQUIRE(cache_pooled && cache_sumw && rows && pooled_raw && sumw, "feature_cache_gather: null argument");
  VLB_REQUIRE(B > 0 && E > 0 && n_rows > 0, "feature_cache_gather: bad shape B=%d E=%d n_rows=%d", B, E, n_rows);
  feature_cache_gather_launch(cache_pooled, cache_sumw, rows, pooled_raw, sumw, B, E, n_rows, as_stream(stream));
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_head_mix_fwd(const float* p_stack, const void* a, float* alpha, float* pooled_raw, int K, int B, int E,
                                void* stream) {
  VLB_REQUIRE(p_stack && alpha && pooled_raw, "head_mix_fwd: null argument");
  VLB_REQUIRE(K >= 1 && K <= MIX_KMAX && B > 0 && E > 0 && E % 8 == 0, "head_mix_fwd: bad shape K=%d B=%d E=%d", K, B, E);
  VLB_REQUIRE(a || K == 1, "head_mix_fwd: K=%d layers need their logits (a is null)", K);
  const int64_t n = (int64_t)B * E;
  hipLaunchKernelGGL(head_mix_fwd_kernel, dim3((unsigned)((n + MIX_CHUNK - 1) / MIX_CHUNK)), dim3(256), 0, as_stream(stream), p_stack,
                     (const bf16*)a, alpha, pooled_raw, K, n);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int64_t vlb_head_mix_ws_floats(int K, int B, int E) {
  return (int64_t)K * (((int64_t)B * E + MIX_CHUNK - 1) / MIX_CHUNK);
}

extern "C" int vlb_head_mix_bwd(const float* p_stack, const float* draw, const float* alpha, float* d_a, float* draw_stack,
                                float* ws, int K, int B, int E, void* stream) {
  VLB_REQUIRE(p_stack && draw && alpha && d_a && draw_stack && ws, "head_mix_bwd: null argument");
  VLB_REQUIRE(K >= 1 && K <= MIX_KMAX && B > 0 && E > 0 && E % 8 == 0, "head_mix_bwd: bad shape K=%d B=%d E=%d", K, B, E);
  hipStream_t st = as_stream(stream);
  const int64_t n = (int64_t)B * E;
  const int nblk = (int)((n + MIX_CHUNK - 1) / MIX_CHUNK);
  hipLaunchKernelGGL(head_mix_bwd_kernel, dim3(nblk), dim3(256), 0, st, p_stack, draw, alpha, ws, draw_stack, K, n);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(head_mix_da_kernel, dim3(1), dim3(64), 0, st, ws, alpha, d_a, K, nblk);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_head_dhidden(const void* hidden, const float* wmask, const float* stats, const float* draw, void* dx, int B,
                                int S, int E, const int* cu_rows, int total_rows, int accumulate, void* stream) {
  VLB_REQUIRE(hidden && wmask && stats && draw && dx, "head_dhidden: null argument");
  VLB_REQUIRE(B > 0 && S > 0 && E % 8 == 0 && E > 0 && E <= 8192, "head_dhidden: bad shape B=%d S=%d E=%d", B, S, E);
  const int64_t rows = cu_rows ? (int64_t)total_rows : (int64_t)B * S;
  VLB_REQUIRE(rows > 0 && rows <= (int64_t)B * S, "head_dhidden: total_rows=%d out of range", total_rows);
  hipStream_t st = as_stream(stream);
  const dim3 grid((unsigned)((rows + 3) / 4));
  if (accumulate) {
    const int ni = (E + 511) / 512;          // <= 16: E <= 8192
#define VLB_DH_ACC(NI) hipLaunchKernelGGL(head_dhidden_acc_kernel<NI>, grid, dim3(256), 0, st, (const bf16*)hidden, wmask, stats, draw, \
                                          (bf16*)dx, S, E, rows, B, cu_rows)
    if (ni <= 1) VLB_DH_ACC(1);
    else if (ni <= 2) VLB_DH_ACC(2);
    else if (ni <= 4) VLB_DH_ACC(4);
    else if (ni <= 8) VLB_DH_ACC(8);
    else VLB_DH_ACC(16);
#undef VLB_DH_ACC
  } else
    head_dhidden_launch(hidden, wmask, stats, draw, dx, B, S, E, rows, cu_rows, st);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// ---------------------------------------------------------------- per-target loss weights: entry points
namespace {
template <int KIND>
int head_wloss_launch(const float* pred, const float* y, const float* tw, const int* group, const float* lpart, int parts,
                      float* wstat, float* loss_terms, float* loss_aux, int B, int V, float l2_lambda, hipStream_t st) {
  hipLaunchKernelGGL(head_wrowstat_kernel<KIND>, dim3(B), dim3(1024), 0, st, pred, y, tw, group, wstat, V);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(wloss_finalize_kernel, dim3(1), dim3(256), 0, st, lpart, parts, l2_lambda, wstat, B,
                     KIND != VLB_LOSS_MSE ? 1 : 0, loss_terms, loss_aux);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}
template <int KIND>
int head_wdpred_launch(const float* pred, const float* y, const float* tw, const int* group, const float* wstat, float* dpred,
                       int B, int V, float loss_scale, hipStream_t st) {
  hipLaunchKernelGGL(head_wdpred_kernel<KIND>, dim3((V + 255) / 256, B), dim3(256), 0, st, pred, y, tw, group, wstat, dpred, B, V,
                     loss_scale);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}
}  // namespace

extern "C" int vlb_head_wloss_fwd(const float* pred, const float* y, const float* tw, const int* group, const float* ws,
                                  float* wstat, float* loss_terms, float* loss_aux, int B, int S, int E, int V, int G,
                                  int loss_kind, float l2_lambda, void* stream) {
  VLB_REQUIRE(pred && y && tw && ws && wstat && loss_terms && loss_aux, "head_wloss_fwd: null argument");
  VLB_REQUIRE(loss_kind == VLB_LOSS_MSE || loss_kind == VLB_LOSS_COSINE || loss_kind == VLB_LOSS_PEARSON,
              "head_wloss_fwd: unknown loss_kind %d", loss_kind);
  VLB_REQUIRE(B > 0 && B <= 65535 && S >= 0 && V > 0 && G >= 1 && E % 8 == 0 && E > 0 && E <= 8192,
              "head_wloss_fwd: bad shape B=%d S=%d E=%d V=%d G=%d", B, S, E, V, G);
  VLB_REQUIRE(group ? S == 0 : G == 1, "head_wloss_fwd: group goes with S = 0 (the grouped forward), no group with G = 1 (S=%d G=%d)",
              S, G);
  VLB_REQUIRE((int64_t)G * V <= GROUPED_MAX_ROWS, "head_wloss_fwd: G*V = %lld rows, at most 2^27", (long long)G * V);
  VLB_REQUIRE(loss_kind != VLB_LOSS_PEARSON || V >= 2, "head_wloss_fwd: pearson needs V >= 2 (V=%d)", V);
  // where the forward left the ridge partials: behind the pooling slabs (vlb_head_fwd), or at ws (cached / grouped)
  const float* lpart = ws + (S > 0 ? (int64_t)B * vlb_head_partial_rows(S) * (E + 2) : 0);
  const int parts = ridge_fwd_parts(B, E, V, G, ridge_fwd_is_mfma(B, E));
  hipStream_t st = as_stream(stream);
  if (loss_kind == VLB_LOSS_PEARSON)
    return head_wloss_launch<VLB_LOSS_PEARSON>(pred, y, tw, group, lpart, parts, wstat, loss_terms, loss_aux, B, V, l2_lambda, st);
  if (loss_kind == VLB_LOSS_COSINE)
    return head_wloss_launch<VLB_LOSS_COSINE>(pred, y, tw, group, lpart, parts, wstat, loss_terms, loss_aux, B, V, l2_lambda, st);
  return head_wloss_launch<VLB_LOSS_MSE>(pred, y, tw, group, lpart, parts, wstat, loss_terms, loss_aux, B, V, l2_lambda, st);
}

extern "C" int vlb_head_bwd_wloss(const void* ln1_w, const void* ln2_w, const void* ridge_w, const float* y, const float* tw,
                                  const float* keep_scale, const int* group, const float* pooled_raw, const float* sumw,
                                  const float* zhat, const float* ln2_rstd, const void* z, const float* pred, const float* wstat,
                                  float* dpred, float* d_ridge_w, float* d_ridge_b, float* d_ln2_w, float* d_ln2_b, float* d_ln1_w,
                                  float* d_ln1_b, float* ws, float* dz_ws, float* dpooled_ws, int B, int E, int V, int G,
                                  float l2_lambda, float loss_scale, float l2_scale, int loss_kind, void* stream) {
  VLB_REQUIRE(ln1_w && ln2_w && ridge_w && y && tw && pooled_raw && sumw && zhat && ln2_rstd && z && pred && wstat && dpred &&
                  d_ridge_w && d_ridge_b && d_ln2_w && d_ln2_b && d_ln1_w && d_ln1_b && ws && dz_ws && dpooled_ws,
              "head_bwd_wloss: null argument");
  VLB_REQUIRE(loss_kind == VLB_LOSS_MSE || loss_kind == VLB_LOSS_COSINE || loss_kind == VLB_LOSS_PEARSON,
              "head_bwd_wloss: unknown loss_kind %d", loss_kind);
  VLB_REQUIRE(B > 0 && B <= 65535 && V > 0 && G >= 1 && E % 8 == 0 && E > 0 && E <= 8192,
              "head_bwd_wloss: bad shape B=%d E=%d V=%d G=%d", B, E, V, G);
  VLB_REQUIRE(group || G == 1, "head_bwd_wloss: G = %d heads need group", G);
  VLB_REQUIRE((int64_t)G * V <= GROUPED_MAX_ROWS, "head_bwd_wloss: G*V = %lld rows, at most 2^27", (long long)G * V);
  VLB_REQUIRE(loss_kind != VLB_LOSS_PEARSON || V >= 2, "head_bwd_wloss: pearson needs V >= 2 (V=%d)", V);
  hipStream_t st = as_stream(stream);
  int rc;
  if (loss_kind == VLB_LOSS_PEARSON) rc = head_wdpred_launch<VLB_LOSS_PEARSON>(pred, y, tw, group, wstat, dpred, B, V, loss_scale, st);
  else if (loss_kind == VLB_LOSS_COSINE) rc = head_wdpred_launch<VLB_LOSS_COSINE>(pred, y, tw, group, wstat, dpred, B, V, loss_scale, st);
  else rc = head_wdpred_launch<VLB_LOSS_MSE>(pred, y, tw, group, wstat, dpred, B, V, loss_scale, st);
  if (rc != VLB_OK) return rc;
  // everything behind d pred: the existing launches, reading the buffer where they re-derived it
  return head_bwd_params(ln1_w, ln2_w, ridge_w, y, keep_scale, group, pooled_raw, sumw, zhat, ln2_rstd, z, dpred, d_ridge_w, d_ridge_b,
                         d_ln2_w, d_ln2_b, d_ln1_w, d_ln1_b, ws, dz_ws, dpooled_ws, nullptr, B, E, V, group ? G : 1, l2_lambda,
                         loss_scale, l2_scale, LOSS_FROM_DPRED, stream);
}

// ---------------------------------------------------------------- the exported layers on their own
extern "C" int64_t vlb_hrf_pool_ws_floats(int B, int E) { return (int64_t)B * HRF_SPLITS * E; }

extern "C" int vlb_hrf_pool(const void* embeddings, int emb_is_f32, const float* weights, void* out, float* ws, int B, int S, int E,
                            void* stream) {
  VLB_REQUIRE(embeddings && weights && out && ws && B > 0 && S > 0 && E > 0 && E % 8 == 0, "hrf_pool: bad arguments (E must be a multiple of 8)");
  hipStream_t st = as_stream(stream);
  const dim3 grid(HRF_SPLITS, (E + 511) / 512, B), rgrid((E + 255) / 256, B);
  if (emb_is_f32) {
    hipLaunchKernelGGL(hrf_pool_kernel<float>, grid, dim3(256), 0, st, (const float*)embeddings, weights, ws, S, E);
    VLB_LAUNCH_CHECK();
    hipLaunchKernelGGL(hrf_pool_reduce_kernel<float>, rgrid, dim3(256), 0, st, ws, (float*)out, E);
  } else {
    hipLaunchKernelGGL(hrf_pool_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)embeddings, weights, ws, S, E);
    VLB_LAUNCH_CHECK();
    hipLaunchKernelGGL(hrf_pool_reduce_kernel<bf16>, rgrid, dim3(256), 0, st, ws, (bf16*)out, E);
  }
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int64_t vlb_ridge_ws_floats(int V) { return 2 * (int64_t)((V + RIDGE_ROWS - 1) / RIDGE_ROWS) + 8; }

extern "C" int vlb_ridge_fwd(const void* x, const void* ridge_w, const void* ridge_b, float* pred, float* l2_out, float* ws, int B, int E,
                             int V, float l2_lambda, void* stream) {
  VLB_REQUIRE(x && ridge_w && ridge_b && pred && l2_out && ws && B > 0 && V > 0 && E > 0 && E % 8 == 0, "ridge_fwd: bad arguments");
  hipStream_t st = as_stream(stream);
  // y = nullptr: no error term.  The layer on its own always runs the scalar form: its bits do not depend on (B, E).
  const int rblk = ridge_fwd_launch(ridge_w, ridge_b, x, nullptr, nullptr, pred, ws, B, E, V, 1, false, st);
  if (rblk < 0) return rblk;
  float* terms = ws + 2 * (int64_t)rblk;
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, st, ws, rblk, 1.f / ((float)B * (float)V), l2_lambda, terms);
  VLB_LAUNCH_CHECK();
  hipError_t e = hipMemcpyAsync(l2_out, terms + 1, sizeof(float), hipMemcpyDeviceToDevice, st);
  if (e != hipSuccess) { vlb_set_error("ridge_fwd: copy failed: %s", hipGetErrorString(e)); return VLB_ERR_LAUNCH; }
  return VLB_OK;
}

// ---------------------------------------------------------------- per-row ridge penalty
// With one l2_lambda per row of ridge_layer.linear.weight (R = max(1,G) V rows) the penalty is sum_r lam[r] ||W_r||^2.  The
// existing entries are handed l2_lambda = 0 (their l2 term and l2 gradient are exactly zero) and these two run after them on
// the same stream.  Both stream W once: a lane reads 8 bf16 as one 16-byte load, the 64 lanes of a wave 1 KiB contiguous.
namespace {

constexpr int L2R_MAX_BLOCKS = 2048;      // memory-bound grid cap: 256 CUs x 8 blocks; the rest is grid-strided

// forward, stage 1: a wave owns rows gw, gw + nw, ... (gw = its index in the grid, nw = waves in the grid) in ascending order.
// Per row: each lane adds the fp32 squares (exact: a bf16 square has 16 significant bits) of its chunks lane, lane + 64, ...
// into one fp64 accumulator, the 64 lanes are summed by a fixed xor butterfly, the row sum is multiplied by (double)lam[r] and
// added to the wave's fp64 total.  part[block] = the 4 waves' totals in ascending order.  No atomics.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void l2_rows_partial_kernel(const bf16* __restrict__ W, const float* __restrict__ lam,
                                                              double* __restrict__ part, int R, int E) {
  __shared__ double wtot[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = gridDim.x * 4, chunks = E >> 3;
  double total = 0.0;
  for (int r = blockIdx.x * 4 + wave; r < R; r += nw) {
    const bf16* row = W + (int64_t)r * E;
    double s = 0.0;
#pragma unroll 4
    for (int c = lane; c < chunks; c += 64) {
      const bf16x8 w = *reinterpret_cast<const bf16x8*>(row + 8 * c);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)w[j];
        s += (double)(f * f);
      }
    }
    s = wave_sum_f64(s);
    total += (double)lam[r] * s;
  }
  if (lane == 0) wtot[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((wtot[0] + wtot[1]) + wtot[2]) + wtot[3];
}

// forward, stage 2 (one block, in the mould of loss_finalize_kernel): thread i sums partials i, i + 256, ... in order, the 256
// sums are tree-summed in LDS; loss_terms[1] <- the total rounded once to fp32, loss_terms[2] <- loss_terms[0] + loss_terms[1]
__global__ __launch_bounds__(256) void l2_rows_finish_kernel(const double* __restrict__ part, int nblk, float* __restrict__ out) {
  __shared__ double sm[256];
  double t = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 256) t += part[i];
  sm[threadIdx.x] = t;
  __syncthreads();
  for (int s2 = 128; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) sm[threadIdx.x] += sm[threadIdx.x + s2];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float l2 = (float)sm[0];
    out[1] = l2;
    out[2] = out[0] + l2;
  }
}

// backward: d[r,e] += (coef lam[r]) (float)W[r,e], one owner per element: a thread takes 8 consecutive elements of one row
// (one 16-byte load of W, two 16-byte loads and stores of d).  A row with lam[r] == 0 is neither read nor written.
__global__ __launch_bounds__(256) void l2_rows_bwd_kernel(const bf16* __restrict__ W, const float* __restrict__ lam,
                                                          float* __restrict__ d, int64_t nchunks, int chunks_per_row, float coef) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < nchunks; c += stride) {
    const float l = lam[c / chunks_per_row];
    if (l == 0.f) continue;
    const float k = coef * l;
    const bf16x8 w = *reinterpret_cast<const bf16x8*>(W + 8 * c);
    f32x4* dp = reinterpret_cast<f32x4*>(d + 8 * c);
    f32x4 lo = dp[0], hi = dp[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      lo[j] = fmaf(k, (float)w[j], lo[j]);
      hi[j] = fmaf(k, (float)w[4 + j], hi[j]);
    }
    dp[0] = lo;
    dp[1] = hi;
  }
}

inline int l2_rows_blocks(int R) {
  const int b = (R + 3) / 4;
  return b < L2R_MAX_BLOCKS ? b : L2R_MAX_BLOCKS;
}

}  // namespace

extern "C" int64_t vlb_head_l2_rows_ws_doubles(int R) { return R < 1 ? 0 : (int64_t)l2_rows_blocks(R); }

extern "C" int vlb_head_l2_rows_fwd(const void* ridge_w, const float* lam, double* ws, float* loss_terms, int R, int E,
                                    void* stream) {
  VLB_REQUIRE(ridge_w && lam && ws && loss_terms, "head_l2_rows_fwd: null argument");
  VLB_REQUIRE(R >= 1 && E >= 8 && E % 8 == 0 && E <= 8192, "head_l2_rows_fwd: bad shape R=%d E=%d (E %% 8 == 0, E <= 8192)", R, E);
  VLB_REQUIRE(((uintptr_t)ridge_w & 15) == 0, "head_l2_rows_fwd: ridge_w is not 16-byte aligned");
  hipStream_t st = as_stream(stream);
  const int nblk = l2_rows_blocks(R);
  hipLaunchKernelGGL(l2_rows_partial_kernel, dim3(nblk), dim3(256), 0, st, (const bf16*)ridge_w, lam, ws, R, E);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(l2_rows_finish_kernel, dim3(1), dim3(256), 0, st, ws, nblk, loss_terms);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_head_l2_rows_bwd(const void* ridge_w, const float* lam, float* d_ridge_w, int R, int E, float coef,
                                    void* stream) {
  VLB_REQUIRE(ridge_w && lam && d_ridge_w, "head_l2_rows_bwd: null argument");
  VLB_REQUIRE(R >= 1 && E >= 8 && E % 8 == 0 && E <= 8192, "head_l2_rows_bwd: bad shape R=%d E=%d (E %% 8 == 0, E <= 8192)", R, E);
  VLB_REQUIRE(((uintptr_t)ridge_w & 15) == 0 && ((uintptr_t)d_ridge_w & 15) == 0, "head_l2_rows_bwd: a tensor is not 16-byte aligned");
  const int64_t nchunks = (int64_t)R * (E >> 3);
  const int64_t want = (nchunks + 255) / 256;
  const int nblk = (int)(want < L2R_MAX_BLOCKS ? want : L2R_MAX_BLOCKS);
  hipLaunchKernelGGL(l2_rows_bwd_kernel, dim3(nblk), dim3(256), 0, as_stream(stream), (const bf16*)ridge_w, lam, d_ridge_w, nchunks,
                     E >> 3, coef);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}
