// Held-out scoring of the brain head: per-target r, R^2 and MSE from five fp64 running sums kept per block
// of clips, and a block bootstrap over those blocks.  The sums are the ones the reference's LogValAccuracyCallback needs
// (src/utils.py:85-110), kept on the device per (head, block) instead of per epoch.
//
// Rules of every kernel here: fp64 arithmetic, no atomics, one owning thread and one summation order per output element,
// adjacent lanes on adjacent targets (every load and store is contiguous over the lanes), 64-bit indices.  Contraction is
// off: every product, quotient and sum is rounded once, in the order written, so a host loop in the same order gives the
// same bits (tests/score_emul.py).
#include "common.hpp"

#pragma clang fp contract(off)

namespace {

// keep[v] > 0 through a select: a masked target's pred / y are never read into arithmetic
__device__ __forceinline__ bool kept_target(const float* __restrict__ keep, int64_t i) { return keep == nullptr || keep[i] > 0.f; }

// sums[slot[b], :, v] += (p, y, p p, y y, p y) for b ascending.  One thread per target; the five sums of the current slot stay
// in registers while consecutive clips share it (loaded when the slot changes, stored when it changes again or at the end),
// which is the same chain of additions as a read-modify-write per clip.  The fp32 values are widened first, so the three
// products are exact.  A slot outside [0, n_slots) (the caller checks on the host) is skipped, never written.
__global__ __launch_bounds__(256) void score_accumulate_kernel(const float* __restrict__ pred, int64_t ldp,
                                                               const float* __restrict__ y, int64_t ldy,
                                                               const int* __restrict__ slot, const float* __restrict__ keep,
                                                               double* __restrict__ sums, int B, int64_t V, int nb, int n_slots) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  int cur = -1;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
  double* at = nullptr;
  for (int b = 0; b < B; ++b) {
    const int sl = slot[b];                               // wave-uniform
    if (sl < 0 || sl >= n_slots) continue;
    if (sl != cur) {
      if (at != nullptr) { at[0] = s0; at[V] = s1; at[2 * V] = s2; at[3 * V] = s3; at[4 * V] = s4; }
      cur = sl;
      at = sums + (int64_t)sl * 5 * V + v;
      s0 = at[0]; s1 = at[V]; s2 = at[2 * V]; s3 = at[3 * V]; s4 = at[4 * V];
    }
    const bool k = kept_target(keep, (int64_t)(sl / nb) * V + v);
    const float pf = pred[(int64_t)b * ldp + v], yf = y[(int64_t)b * ldy + v];
    const double p = k ? (double)pf : 0.0, t = k ? (double)yf : 0.0;
    s0 += p; s1 += t; s2 += p * p; s3 += t * t; s4 += p * t;
  }
  if (at != nullptr) { at[0] = s0; at[V] = s1; at[2 * V] = s2; at[3 * V] = s3; at[4 * V] = s4; }
}

// Pearson r from five totals and the clip count: vlb_ridge_cv_score's rule (0 unless both variances are positive, clipped)
__device__ __forceinline__ double score_r(double tp, double ty, double tpp, double tyy, double tpy, double n) {
  const double cov = tpy - tp * ty / n;
  const double vp = tpp - tp * tp / n;
  const double vy = tyy - ty * ty / n;
  double r = 0.0;
  if (vp > 0.0 && vy > 0.0) {
    r = cov / sqrt(vp * vy);
    r = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;
  }
  return r;
}

// out[0..3, v] = r, R^2, mse, n from T = sum_j sums_h[j] (j ascending, from 0) and n = sum_j n_j; NaN in out[0..2] where masked
__global__ __launch_bounds__(256) void score_finish_kernel(const double* __restrict__ sums_h, const double* __restrict__ n_j, int nb,
                                                           const float* __restrict__ keep_h, double* __restrict__ out, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  double n = 0.0, t[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < nb; ++j) {
    n += n_j[j];
#pragma unroll
    for (int k = 0; k < 5; ++k) t[k] += sums_h[((int64_t)j * 5 + k) * V + v];
  }
  out[3 * V + v] = n;
  if (!kept_target(keep_h, v)) {
    const double nan = __builtin_nan("");
    out[v] = nan; out[V + v] = nan; out[2 * V + v] = nan;
    return;
  }
  const double vy = t[3] - t[1] * t[1] / n;
  const double sse = t[2] - 2.0 * t[4] + t[3];
  out[v] = score_r(t[0], t[1], t[2], t[3], t[4], n);
  out[V + v] = vy > 0.0 ? 1.0 - sse / vy : 0.0;
  out[2 * V + v] = sse / n;
}

// avg[c] = mean over the kept targets of out[c, :], c = 0..2: thread t adds v = t, t + 256, ... in ascending order, thread 0
// adds the 256 partials in ascending order (ridge_finish_kernel's pattern).  One block.  No kept target: NaN.
__global__ __launch_bounds__(256) void score_avg_kernel(const double* __restrict__ out, const float* __restrict__ keep_h,
                                                        double* __restrict__ avg, int64_t V) {
  __shared__ double part[4][256];
  double s[3] = {0.0, 0.0, 0.0}, c = 0.0;
  for (int64_t v = threadIdx.x; v < V; v += 256) {
    if (!kept_target(keep_h, v)) continue;
    c += 1.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += out[(int64_t)k * V + v];
  }
  part[0][threadIdx.x] = s[0]; part[1][threadIdx.x] = s[1]; part[2][threadIdx.x] = s[2]; part[3][threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < 256; ++i)
      for (int k = 0; k < 4; ++k) a[k] += part[k][i];
    for (int k = 0; k < 3; ++k) avg[k] = a[k] / a[3];          // 0 / 0 = NaN: nothing kept
  }
}

// Block bootstrap.  A thread owns one target and walks the R resamples in tiles of RT: the tile's 5 RT totals stay in registers
// while the nb draws of each of its resamples are added in index order (T = sum_k sums_h[draws[rho, k]], pure additions, and
// the clip count the same way), so RT x 5 independent loads are in flight per step of k.  draws is indexed by kernel arguments
// and loop counters only: the loads are wave-uniform.  A draw outside [0, nb) (the caller checks on the host) is clamped, never
// followed.  r* by score_r; the mean and the spread are accumulated in rho order on d = r* - r*_0 (the first resample's
// value: the variance does not depend on the shift, and equal r* - a head with one block - give a spread of exactly 0).
constexpr int RT = 8;
__global__ __launch_bounds__(64) void score_bootstrap_kernel(const double* __restrict__ sums_h, const double* __restrict__ n_j,
                                                             int nb, const int* __restrict__ draws, int R,
                                                             const float* __restrict__ keep_h, double* __restrict__ out, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (v >= V) return;
  if (!kept_target(keep_h, v)) {
    const double nan = __builtin_nan("");
    out[v] = nan; out[V + v] = nan; out[2 * V + v] = nan;
    return;
  }
  const double* __restrict__ col = sums_h + v;
  double r0 = 0.0, s1 = 0.0, s2 = 0.0;
  int le0 = 0;
  for (int rho0 = 0; rho0 < R; rho0 += RT) {
    double t[RT][5], n[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      n[i] = 0.0;
#pragma unroll
      for (int k = 0; k < 5; ++k) t[i][k] = 0.0;
    }
    for (int k = 0; k < nb; ++k) {
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const int rho = rho0 + i < R ? rho0 + i : R - 1;        // a short last tile repeats the last resample, unused below
        int j = draws[(int64_t)rho * nb + k];
        j = j < 0 ? 0 : j >= nb ? nb - 1 : j;
        n[i] += n_j[j];
        const double* __restrict__ at = col + (int64_t)j * 5 * V;
#pragma unroll
        for (int c = 0; c < 5; ++c) t[i][c] += at[(int64_t)c * V];
      }
    }
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      if (rho0 + i < R) {
        const double r = score_r(t[i][0], t[i][1], t[i][2], t[i][3], t[i][4], n[i]);
        if (rho0 + i == 0) r0 = r;
        const double d = r - r0;
        s1 += d;
        s2 += d * d;
        le0 += r <= 0.0 ? 1 : 0;
      }
    }
  }
  const double Rd = (double)R;
  const double var = (s2 - s1 * s1 / Rd) / (Rd - 1.0);
  out[v] = r0 + s1 / Rd;
  out[V + v] = sqrt(var > 0.0 ? var : 0.0);
  out[2 * V + v] = (1.0 + (double)le0) / (Rd + 1.0);
}

}  // namespace

// ---------------------------------------------------------------- C-ABI
extern "C" int vlb_score_accumulate(const float* pred, int ldp, const float* y, int ldy, const int* slot, const float* keep,
                                    double* sums, int B, int V, int nb, int n_slots, void* stream) {
  VLB_REQUIRE(pred && y && slot && sums, "score_accumulate: null argument");
  VLB_REQUIRE(B >= 1 && V >= 1 && ldp >= V && ldy >= V, "score_accumulate: bad shape B=%d V=%d ldp=%d ldy=%d", B, V, ldp, ldy);
  VLB_REQUIRE(nb >= 1 && n_slots >= 1 && n_slots % nb == 0, "score_accumulate: bad slots nb=%d n_slots=%d (n_slots must be a "
              "positive multiple of nb)", nb, n_slots);
  hipLaunchKernelGGL(score_accumulate_kernel, dim3((V + 255) / 256), dim3(256), 0, as_stream(stream), pred, (int64_t)ldp, y,
                     (int64_t)ldy, slot, keep, sums, B, (int64_t)V, nb, n_slots);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_score_finish(const double* sums_h, const double* n_j, int nb, const float* keep_h, double* out, double* avg,
                                int V, void* stream) {
  VLB_REQUIRE(sums_h && n_j && out && avg, "score_finish: null argument");
  VLB_REQUIRE(nb >= 1 && V >= 1, "score_finish: bad shape nb=%d V=%d", nb, V);
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(score_finish_kernel, dim3((V + 255) / 256), dim3(256), 0, st, sums_h, n_j, nb, keep_h, out, (int64_t)V);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(score_avg_kernel, dim3(1), dim3(256), 0, st, out, keep_h, avg, (int64_t)V);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_score_bootstrap(const double* sums_h, const double* n_j, int nb, const int* draws, int R, const float* keep_h,
                                   double* out, int V, void* stream) {
  VLB_REQUIRE(sums_h && n_j && draws && out, "score_bootstrap: null argument");
  VLB_REQUIRE(nb >= 1 && V >= 1, "score_bootstrap: bad shape nb=%d V=%d", nb, V);
  VLB_REQUIRE(R >= 2, "score_bootstrap: R=%d resamples, at least 2 are needed", R);
  hipLaunchKernelGGL(score_bootstrap_kernel, dim3((V + 63) / 64), dim3(64), 0, as_stream(stream), sums_h, n_j, nb, draws, R, keep_h,
                     out, (int64_t)V);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}
