// Grouped clip + AdamW (vlb_adamw_step_groups in ops.hip: fp32 gradients; vlb_adamw_step_groups_g16 in train.hip: bf16
// gradients): ONE launch over a flat store whose element ranges carry their own learning rate and weight decay
// (litmodule.config.optimizer_groups).
//
// The per-element arithmetic is adamw_kernel's / adamw4's, operation for operation (see adamw_groups4), so a grouped step is
// bit-identical to one parent launch per range with that range's (lr, weight_decay).  What differs is where a lane gets the
// two rates from:
//   * `bounds` (int64, ascending, bounds[0] = 0, bounds[n_ranges] = n, every entry a multiple of 8) and `group_of` (int32,
//     one group per range) are device arrays built once by optim_groups.group_ranges; a lane owns 4 consecutive elements, which never
//     straddle a boundary, and finds its range by binary search.  Tables of up to kAdamwLdsRanges ranges are copied into LDS
//     once per workgroup (the 7B LoRA store has 8 ranges per decoder layer: ~260); longer ones are searched in global memory,
//     where the few lines a workgroup touches stay in L2.  Either way the search runs after the state loads of the trip were
//     issued, i.e. under their HBM latency.
//   * lr[] / weight_decay[] arrive BY VALUE in the kernel argument (they change every scheduler step: no per-step upload, no
//     sync); the group's pair is picked by eight selects on SGPR operands - a dynamic index would put the struct in scratch.
// Memory access is adamw_g16_kernel's: 16-byte lane accesses on master / m / v (and an fp32 gradient), 8 bytes on the bf16
// copy (and a bf16 gradient), two independent chunks in flight per loop trip, the same grid.  No atomics, vector stores only.
//
// EMA (vlb_adamw_step_ema / vlb_adamw_step_groups_ema in ops.hip, fp32 gradients; litmodule.config.ema_decay):
// the same loop with one more fp32 array.  `ema` is loaded with p / m / v / g of its trip (16-byte lanes, the prefetch of the
// next trip included) and ema' = (d * ema) + (omd * p') is stored with them, p' being the master just computed and
// omd = 1 - d; the three operations keep their own roundings (adamw_groups4).  d arrives by value: it changes per step
// during warm-up.  It is adamw_groups_kernel itself with the EMA switched on at compile time; TABLE = false is the ungrouped
// call: one (lr, weight_decay) pair, no table, no search.  The kernels without EMA compile to what they were: every EMA
// statement sits behind `if constexpr`, and the EMA's arguments are a parameter pack that is empty for them.
#pragma once
#include "common.hpp"

constexpr int kAdamwMaxGroups = 8;
constexpr int kAdamwLdsRanges = 512;
struct AdamwGroupRates {
  float lr[kAdamwMaxGroups];
  float wd[kAdamwMaxGroups];
};

__device__ __forceinline__ f32x4 adamw_ld_grad4(const float* g) { return *reinterpret_cast<const f32x4*>(g); }
__device__ __forceinline__ f32x4 adamw_ld_grad4(const bf16* g) {
  const bf16x4 v = *reinterpret_cast<const bf16x4*>(g);
  return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};      // exact widening: (float)gv[k] of adamw4
}

// range r with bounds[r] <= e < bounds[r + 1]   (bounds[0] = 0 <= e < n = bounds[n_ranges])
__device__ __forceinline__ int adamw_find_range(const int64_t* __restrict__ bounds, int n_ranges, int64_t e) {
  int lo = 0, hi = n_ranges;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (bounds[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void adamw_group_rates(const AdamwGroupRates& r, int grp, float& lr, float& wd) {
  lr = r.lr[0]; wd = r.wd[0];
#pragma unroll
  for (int k = 1; k < kAdamwMaxGroups; ++k)
    if (grp == k) { lr = r.lr[k]; wd = r.wd[k]; }
}

// The update of one element:
//     gi = g * clip;  p' = p * (1 - lr * wd);  m' = b1 * m + (1 - b1) * gi;  v' = b2 * v + (1 - b2) * gi * gi;
//     p' -= (lr / bc1) * m' / (sqrtf(v') / bc2_sqrt + eps)
// - adamw_kernel's and adamw4's source line for line.  The compiler contracts those lines into fused multiply-adds, and it
// does so DIFFERENTLY in the two parents (scalar code in adamw_kernel, packed code in adamw4: read from their gfx950 ISA):
//     adamw_kernel (fp32 g):  m' = fma(1 - b1, gi, b1 * m)      v' = fma(gi, (1 - b2) * gi, b2 * v)
//     adamw4       (bf16 g):  m' = fma(b1, m, (1 - b1) * gi)    v' = fma(b2, v, ((1 - b2) * gi) * gi)
//     both:                   p' = fma(fma(-lr, wd, 1), p, -((lr / bc1) * m') / (sqrtf(v') / bc2_sqrt + eps))
// Which product keeps its rounding is visible in the last bit, so each grouped kernel spells out the operations of the parent
// it stands in for (G16 = the gradient type's parent) with contraction switched off, instead of leaving the choice to a third
// run of the same heuristic.  tests/test_gpu_adamw_groups.py holds both to torch.equal against their parents.
// EMA: ema' = (d * ema) + (omd * p') behind the update, one product, one product, one sum, each rounded to fp32 on its own
// (contraction is off in this function), so that a float32 restatement on the host reproduces it bit for bit - a fused
// multiply-add would keep one product unrounded.
template <bool G16, bool EMA = false>
__device__ __forceinline__ void adamw_groups4(float* __restrict__ p, bf16* __restrict__ pb, float* __restrict__ m, float* __restrict__ v,
                                              int64_t i4, float clip, float lr, float b1, float b2, float eps, float wd, float bc1,
                                              float bc2_sqrt, f32x4 pv, f32x4 mv, f32x4 vv, f32x4 gv, float* __restrict__ ema = nullptr,
                                              f32x4 ev = f32x4{}, float d = 0.f, float omd = 0.f) {
#pragma clang fp contract(off)
  bf16x4 o;
  const float decay = __builtin_fmaf(-lr, wd, 1.f), lr_bc = lr / bc1, ob1 = 1.f - b1, ob2 = 1.f - b2;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float gi = gv[k] * clip;
    const float mi = G16 ? __builtin_fmaf(b1, mv[k], ob1 * gi) : __builtin_fmaf(ob1, gi, b1 * mv[k]);
    const float vi = G16 ? __builtin_fmaf(b2, vv[k], (ob2 * gi) * gi) : __builtin_fmaf(gi, ob2 * gi, b2 * vv[k]);
    const float q = (lr_bc * mi) / (sqrtf(vi) / bc2_sqrt + eps);
    const float pi = __builtin_fmaf(decay, pv[k], -q);
    pv[k] = pi; mv[k] = mi; vv[k] = vi; o[k] = (bf16)pi;
    if constexpr (EMA) ev[k] = (d * ev[k]) + (omd * pi);
  }
  *reinterpret_cast<f32x4*>(p + i4 * 4) = pv;
  *reinterpret_cast<f32x4*>(m + i4 * 4) = mv;
  *reinterpret_cast<f32x4*>(v + i4 * 4) = vv;
  if (pb) *reinterpret_cast<bf16x4*>(pb + i4 * 4) = o;
  if constexpr (EMA) *reinterpret_cast<f32x4*>(ema + i4 * 4) = ev;
}

// The EMA's two kernel arguments.  They reach adamw_groups_kernel as a trailing parameter PACK: empty for the kernels without
// EMA, whose signature, kernel-argument layout and generated code therefore stay what they were before the EMA existed.
struct AdamwEma {
  float* ema;
  float d;
};
__device__ __forceinline__ AdamwEma adamw_ema_arg() { return AdamwEma{nullptr, 0.f}; }
__device__ __forceinline__ AdamwEma adamw_ema_arg(AdamwEma e) { return e; }

// TABLE = false (EMA only, LDS = false): no table, rates.lr[0] / rates.wd[0] for every element; bounds / group_of / n_ranges
// are not read.  E: nothing, or one AdamwEma.
template <typename G, bool LDS, bool TABLE = true, typename... E>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, bf16* __restrict__ pb, const G* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t n4,
                                                           const int64_t* __restrict__ bounds, const int32_t* __restrict__ group_of,
                                                           int n_ranges, AdamwGroupRates rates, float b1, float b2, float eps, float bc1,
                                                           float bc2_sqrt, const float* __restrict__ sumsq, float max_norm, E... ema_arg) {
  constexpr bool EMA = sizeof...(E) == 1;
  static_assert(sizeof...(E) <= 1 && (TABLE || !LDS), "one AdamwEma at most; no table: nothing to stage");
  const AdamwEma ea = adamw_ema_arg(ema_arg...);
  float* __restrict__ ema = ea.ema;
  const float d = ea.d, omd = 1.f - d;
  __shared__ int64_t s_bounds[LDS ? kAdamwLdsRanges : 1];
  __shared__ int32_t s_group[LDS ? kAdamwLdsRanges : 1];
  float clip = 1.f;
  if (max_norm > 0.f && sumsq) clip = fminf(1.f, max_norm / (sqrtf(sumsq[0]) + 1e-6f));
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  // first trip's loads go out before the table is staged: the staging and the search run under their latency
  f32x4 p0{}, m0{}, v0{}, g0{}, e0{}, p1{}, m1{}, v1{}, g1{}, e1{};
  auto load = [&](int64_t a, f32x4& pp, f32x4& mm, f32x4& vv, f32x4& gg, f32x4& ee) {
    pp = *reinterpret_cast<const f32x4*>(p + a * 4); mm = *reinterpret_cast<const f32x4*>(m + a * 4);
    vv = *reinterpret_cast<const f32x4*>(v + a * 4); gg = adamw_ld_grad4(g + a * 4);
    if constexpr (EMA) ee = *reinterpret_cast<const f32x4*>(ema + a * 4);
  };
  if (i < n4) load(i, p0, m0, v0, g0, e0);
  if (i + stride < n4) load(i + stride, p1, m1, v1, g1, e1);
  if (LDS) {                      // (entries 0 .. n_ranges - 1 suffice: the search never reads bounds[n_ranges])
    for (int k = threadIdx.x; k < n_ranges; k += 256) { s_bounds[k] = bounds[k]; s_group[k] = group_of[k]; }
    __syncthreads();
  }
  const int64_t* sb = LDS ? s_bounds : bounds;
  const int32_t* sg = LDS ? s_group : group_of;
  for (; i < n4; i += 2 * stride) {
    const int64_t j = i + stride;
    const bool two = j < n4;
    float lr0, wd0, lr1 = 0.f, wd1 = 0.f;
    if constexpr (TABLE) {
      adamw_group_rates(rates, sg[adamw_find_range(sb, n_ranges, i * 4)], lr0, wd0);
      if (two) adamw_group_rates(rates, sg[adamw_find_range(sb, n_ranges, j * 4)], lr1, wd1);
    } else {
      lr0 = lr1 = rates.lr[0]; wd0 = wd1 = rates.wd[0];
    }
    adamw_groups4<sizeof(G) == 2, EMA>(p, pb, m, v, i, clip, lr0, b1, b2, eps, wd0, bc1, bc2_sqrt, p0, m0, v0, g0, ema, e0, d, omd);
    if (two) adamw_groups4<sizeof(G) == 2, EMA>(p, pb, m, v, j, clip, lr1, b1, b2, eps, wd1, bc1, bc2_sqrt, p1, m1, v1, g1, ema, e1, d, omd);
    const int64_t ni = i + 2 * stride;
    if (ni < n4) load(ni, p0, m0, v0, g0, e0);
    if (ni + stride < n4) load(ni + stride, p1, m1, v1, g1, e1);
  }
}

// shared host side of the two entry points; G = float | bf16
template <typename G>
static int adamw_groups_launch(float* master, void* param_bf16, const G* grad, float* m, float* v, int64_t n, const int64_t* bounds,
                               const int32_t* group_of, int n_ranges, const float* lr, const float* weight_decay, int n_groups,
                               float beta1, float beta2, float eps, int step, const float* sumsq, float max_norm, void* stream) {
  VLB_REQUIRE(n > 0 && n % 8 == 0 && master && grad && m && v && step >= 1, "adamw_groups: n must be a positive multiple of 8");
  VLB_REQUIRE(bounds && group_of && lr && weight_decay && n_ranges >= 1 && (int64_t)n_ranges <= n / 8 && n_groups >= 1 &&
                  n_groups <= kAdamwMaxGroups,
              "adamw_groups: 1 <= n_ranges <= n / 8 and 1 <= n_groups <= 8 with their tables are needed");
  VLB_REQUIRE((((uintptr_t)master | (uintptr_t)m | (uintptr_t)v) % 16) == 0 && ((uintptr_t)grad % (4 * sizeof(G))) == 0 &&
                  ((uintptr_t)param_bf16 % 8) == 0 && ((uintptr_t)bounds % 8) == 0 && ((uintptr_t)group_of % 4) == 0,
              "adamw_groups: buffers must be 16-byte (fp32) / 8-byte (bf16) aligned");
  AdamwGroupRates rates;
  for (int k = 0; k < kAdamwMaxGroups; ++k) {          // unused slots repeat group 0: a stray group index stays harmless
    rates.lr[k] = lr[k < n_groups ? k : 0];
    rates.wd[k] = weight_decay[k < n_groups ? k : 0];
  }
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  const int64_t n4 = n / 4;
  int64_t nb = (n4 + 511) / 512; if (nb > 32768) nb = 32768;
  if (n_ranges <= kAdamwLdsRanges)
    hipLaunchKernelGGL((adamw_groups_kernel<G, true>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), master, (bf16*)param_bf16,
                       grad, m, v, n4, bounds, group_of, n_ranges, rates, beta1, beta2, eps, bc1, bc2s, sumsq, max_norm);
  else
    hipLaunchKernelGGL((adamw_groups_kernel<G, false>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), master, (bf16*)param_bf16,
                       grad, m, v, n4, bounds, group_of, n_ranges, rates, beta1, beta2, eps, bc1, bc2s, sumsq, max_norm);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// host side of vlb_adamw_step_ema (TABLE = false: one (lr, weight_decay) pair, bounds / group_of / n_ranges unused) and of
// vlb_adamw_step_groups_ema (TABLE = true: adamw_groups_launch's table contract); fp32 gradients.  A template, so that only
// the source file that calls it (ops.hip) carries the kernels.
template <bool TABLE>
static int adamw_ema_launch(float* master, void* param_bf16, const float* grad, float* m, float* v, float* ema, int64_t n,
                            const int64_t* bounds, const int32_t* group_of, int n_ranges, const float* lr, const float* weight_decay,
                            int n_groups, float beta1, float beta2, float eps, int step, const float* sumsq, float max_norm,
                            float ema_decay, void* stream) {
  VLB_REQUIRE(n > 0 && n % 8 == 0 && master && grad && m && v && ema && step >= 1, "adamw_ema: n must be a positive multiple of 8");
  VLB_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, "adamw_ema: 0 <= ema_decay < 1 is needed");
  VLB_REQUIRE(lr && weight_decay && n_groups >= 1 && n_groups <= kAdamwMaxGroups, "adamw_ema: 1 <= n_groups <= 8 with their rates are needed");
  VLB_REQUIRE(!TABLE || (bounds && group_of && n_ranges >= 1 && (int64_t)n_ranges <= n / 8 && ((uintptr_t)bounds % 8) == 0 &&
                         ((uintptr_t)group_of % 4) == 0),
              "adamw_ema: 1 <= n_ranges <= n / 8 with both tables (8- / 4-byte aligned) is needed");
  VLB_REQUIRE((((uintptr_t)master | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema | (uintptr_t)grad) % 16) == 0 &&
                  ((uintptr_t)param_bf16 % 8) == 0,
              "adamw_ema: buffers must be 16-byte (fp32) / 8-byte (bf16) aligned");
  AdamwGroupRates rates;
  for (int k = 0; k < kAdamwMaxGroups; ++k) {
    rates.lr[k] = lr[k < n_groups ? k : 0];
    rates.wd[k] = weight_decay[k < n_groups ? k : 0];
  }
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  const int64_t n4 = n / 4;
  int64_t nb = (n4 + 511) / 512; if (nb > 32768) nb = 32768;
  bf16* pb = (bf16*)param_bf16;
  const AdamwEma ea{ema, ema_decay};
  if (!TABLE)
    hipLaunchKernelGGL((adamw_groups_kernel<float, false, false, AdamwEma>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), master,
                       pb, grad, m, v, n4, bounds, group_of, n_ranges, rates, beta1, beta2, eps, bc1, bc2s, sumsq, max_norm, ea);
  else if (n_ranges <= kAdamwLdsRanges)
    hipLaunchKernelGGL((adamw_groups_kernel<float, true, true, AdamwEma>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), master,
                       pb, grad, m, v, n4, bounds, group_of, n_ranges, rates, beta1, beta2, eps, bc1, bc2s, sumsq, max_norm, ea);
  else
    hipLaunchKernelGGL((adamw_groups_kernel<float, false, true, AdamwEma>), dim3((unsigned)nb), dim3(256), 0, as_stream(stream), master,
                       pb, grad, m, v, n4, bounds, group_of, n_ranges, rates, beta1, beta2, eps, bc1, bc2s, sumsq, max_norm, ea);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}
