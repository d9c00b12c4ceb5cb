// Fused clip + AdamW: ONE update function (adamw_update), ONE kernel template (adamw_kernel), ONE host launcher
// (adamw_launch) behind the six entry points
//     vlb_adamw_step        vlb_adamw_step_groups        vlb_adamw_step_ema          (fp32 gradients)
//     vlb_adamw_step_g16    vlb_adamw_step_groups_g16    vlb_adamw_step_groups_ema   (_g16: bf16 gradients; EMA: fp32 only)
// over a flat store: fp32 master and moments, an optional bf16 compute copy refreshed in the same pass, the global-norm clip
// read on the device.  What the entry points choose between is where a lane gets (lr, weight_decay) from and whether a
// moving average rides along; the arithmetic and the loop are the same.
//
// Rates.  lr[] / weight_decay[] of up to kAdamwMaxGroups groups arrive BY VALUE in the kernel argument (they
// change every scheduler step: no per-step upload, no sync).  Without a table every element takes pair 0.  With one
// (litmodule.config.optimizer_groups), `bounds` (int64, ascending, bounds[0] = 0, bounds[n_ranges] = n, every entry a multiple
// of 8) and `group_of` (int32, one group per range) are device arrays built once by optim_groups.group_ranges; a lane's 4
// consecutive elements never straddle a boundary and it finds its range by binary search.  Tables of up to kAdamwLdsRanges
// ranges are copied into LDS once per workgroup (the 7B LoRA store has 8 ranges per decoder layer: ~260); longer ones are
// searched in global memory, where the few lines a workgroup touches stay in L2.  Either way the search runs after the state
// loads of the trip were issued, i.e. under their HBM latency.  The group's pair is picked by eight selects on SGPR operands -
// a dynamic index would put the struct in scratch.
//
// Memory access.  A lane owns W consecutive elements.  W = 4: 16-byte lane accesses on master / m / v / ema (and an fp32
// gradient), 8 bytes on the bf16 copy (and a bf16 gradient); two independent chunks in flight per loop trip, the next trip's
// loads issued behind this trip's stores; min(ceil(lanes / 512), 32768) workgroups of 256.  W = 1 is the same kernel for the
// calls vlb_adamw_step alone accepts (n % 8 != 0, or pointers aligned to their element only).  No atomics, vector stores only.
//
// EMA (litmodule.config.ema_decay): one more fp32 array, loaded with p / m / v / g of its trip and stored with
// them as ema' = (d * ema) + (omd * p'), p' being the master just computed and omd = 1 - d.  d arrives by value: it changes
// per step during warm-up.  Every EMA statement sits behind `if constexpr`; the kernels without it never touch `ema`.
#include "common.hpp"

namespace {

constexpr int kAdamwMaxGroups = 8;
constexpr int kAdamwLdsRanges = 512;
struct AdamwGroupRates {
  float lr[kAdamwMaxGroups];
  float wd[kAdamwMaxGroups];
};
enum AdamwTable { kAdamwNoTable, kAdamwLdsTable, kAdamwGlobalTable };

template <typename T, int W>
using adamw_vec = T __attribute__((ext_vector_type(W)));

template <int W>
__device__ __forceinline__ adamw_vec<float, W> adamw_ld_grad(const float* g) { return *reinterpret_cast<const adamw_vec<float, W>*>(g); }
template <int W>
__device__ __forceinline__ adamw_vec<float, W> adamw_ld_grad(const bf16* g) {
  const adamw_vec<bf16, W> v = *reinterpret_cast<const adamw_vec<bf16, W>*>(g);
  adamw_vec<float, W> r;
#pragma unroll
  for (int k = 0; k < W; ++k) r[k] = (float)v[k];      // exact widening
  return r;
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

// THE DEFINITION of the optimiser's bits - the only place in the device source where the update is written.  In real numbers
//     gi = g * clip;  m' = b1 * m + (1 - b1) * gi;  v' = b2 * v + (1 - b2) * gi * gi;
//     p' = p * (1 - lr * wd) - (lr / bc1) * m' / (sqrtf(v') / bc2_sqrt + eps)
// and in fp32, with contraction OFF in this function so that every fused multiply-add and every rounding is the one written:
//     fp32 gradients (G16 = false):  m' = fma(1 - b1, gi, b1 * m)      v' = fma(gi, (1 - b2) * gi, b2 * v)
//     bf16 gradients (G16 = true):   m' = fma(b1, m, (1 - b1) * gi)    v' = fma(b2, v, ((1 - b2) * gi) * gi)
//     both:                          p' = fma(fma(-lr, wd, 1), p, -((lr / bc1) * m') / (sqrtf(v') / bc2_sqrt + eps))
// Which product of a moment keeps its rounding is visible in the last bit, and the two gradient types differ in it for no
// reason but history: each order is what the compiler of the day made of the plain source line in the kernel that first
// served that gradient type (a scalar kernel for fp32, a packed one for bf16).  Checkpoints and runs exist that continue bit
// for bit only on these orders, so both are kept, spelled out, and no longer any compiler's choice.
// tests/golden/adamw_parent_bits.json anchors them (tests/test_gpu_adamw_bits.py).
// EMA: ema' = (d * ema) + (omd * p') behind the update: one product, one product, one sum, each rounded to fp32 on its own,
// so that a float32 restatement on the host (tests/ema_emul.py) reproduces it bit for bit - a fused multiply-add would keep
// one product unrounded.
// Stores the lane's W elements at element offset e.
template <bool G16, int W, bool EMA>
__device__ __forceinline__ void adamw_update(float* __restrict__ p, bf16* __restrict__ pb, float* __restrict__ m, float* __restrict__ v,
                                             float* __restrict__ ema, int64_t e, float clip, float lr, float b1, float b2, float eps,
                                             float wd, float bc1, float bc2_sqrt, float d, float omd, adamw_vec<float, W> pv,
                                             adamw_vec<float, W> mv, adamw_vec<float, W> vv, adamw_vec<float, W> gv,
                                             adamw_vec<float, W> ev) {
#pragma clang fp contract(off)
  adamw_vec<bf16, W> o;
  const float decay = __builtin_fmaf(-lr, wd, 1.f), lr_bc = lr / bc1, ob1 = 1.f - b1, ob2 = 1.f - b2;
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const float gi = gv[k] * clip;
    const float mi = G16 ? __builtin_fmaf(b1, mv[k], ob1 * gi) : __builtin_fmaf(ob1, gi, b1 * mv[k]);
    const float vi = G16 ? __builtin_fmaf(b2, vv[k], (ob2 * gi) * gi) : __builtin_fmaf(gi, ob2 * gi, b2 * vv[k]);
    const float q = (lr_bc * mi) / (sqrtf(vi) / bc2_sqrt + eps);
    const float pi = __builtin_fmaf(decay, pv[k], -q);
    pv[k] = pi; mv[k] = mi; vv[k] = vi; o[k] = (bf16)pi;
    if constexpr (EMA) ev[k] = (d * ev[k]) + (omd * pi);
  }
  *reinterpret_cast<adamw_vec<float, W>*>(p + e) = pv;
  *reinterpret_cast<adamw_vec<float, W>*>(m + e) = mv;
  *reinterpret_cast<adamw_vec<float, W>*>(v + e) = vv;
  if (pb) *reinterpret_cast<adamw_vec<bf16, W>*>(pb + e) = o;
  if constexpr (EMA) *reinterpret_cast<adamw_vec<float, W>*>(ema + e) = ev;
}

// G: gradient type (float | bf16).  W: elements per lane (4 | 1); `lanes` = n / W.  TABLE: kAdamwNoTable - rates.lr[0] /
// rates.wd[0] for every element, bounds / group_of / n_ranges are not read; else the range table, staged in LDS or not.
// EMA = false: ema / d are not read.
template <typename G, int W, AdamwTable TABLE, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, bf16* __restrict__ pb, const G* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v, int64_t lanes,
                                                    const int64_t* __restrict__ bounds, const int32_t* __restrict__ group_of,
                                                    int n_ranges, AdamwGroupRates rates, float b1, float b2, float eps, float bc1,
                                                    float bc2_sqrt, const float* __restrict__ sumsq, float max_norm,
                                                    float* __restrict__ ema, float d) {
  using vecf = adamw_vec<float, W>;
  constexpr bool LDS = TABLE == kAdamwLdsTable;
  const float omd = 1.f - d;
  __shared__ int64_t s_bounds[LDS ? kAdamwLdsRanges : 1];
  __shared__ int32_t s_group[LDS ? kAdamwLdsRanges : 1];
  float clip = 1.f;
  if (max_norm > 0.f && sumsq) clip = fminf(1.f, max_norm / (sqrtf(sumsq[0]) + 1e-6f));
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  // first trip's loads go out before the table is staged: the staging and the search run under their latency
  vecf p0{}, m0{}, v0{}, g0{}, e0{}, p1{}, m1{}, v1{}, g1{}, e1{};
  auto load = [&](int64_t a, vecf& pp, vecf& mm, vecf& vv, vecf& gg, vecf& ee) {
    pp = *reinterpret_cast<const vecf*>(p + a * W); mm = *reinterpret_cast<const vecf*>(m + a * W);
    vv = *reinterpret_cast<const vecf*>(v + a * W); gg = adamw_ld_grad<W>(g + a * W);
    if constexpr (EMA) ee = *reinterpret_cast<const vecf*>(ema + a * W);
  };
  if (i < lanes) load(i, p0, m0, v0, g0, e0);
  if (i + stride < lanes) load(i + stride, p1, m1, v1, g1, e1);
  if (LDS) {                      // (entries 0 .. n_ranges - 1 suffice: the search never reads bounds[n_ranges])
    for (int k = threadIdx.x; k < n_ranges; k += 256) { s_bounds[k] = bounds[k]; s_group[k] = group_of[k]; }
    __syncthreads();
  }
  const int64_t* sb = LDS ? s_bounds : bounds;
  const int32_t* sg = LDS ? s_group : group_of;
  for (; i < lanes; i += 2 * stride) {
    const int64_t j = i + stride;
    const bool two = j < lanes;
    float lr0, wd0, lr1 = 0.f, wd1 = 0.f;
    if constexpr (TABLE != kAdamwNoTable) {
      adamw_group_rates(rates, sg[adamw_find_range(sb, n_ranges, i * W)], lr0, wd0);
      if (two) adamw_group_rates(rates, sg[adamw_find_range(sb, n_ranges, j * W)], lr1, wd1);
    } else {
      lr0 = lr1 = rates.lr[0]; wd0 = wd1 = rates.wd[0];
    }
    adamw_update<sizeof(G) == 2, W, EMA>(p, pb, m, v, ema, i * W, clip, lr0, b1, b2, eps, wd0, bc1, bc2_sqrt, d, omd, p0, m0, v0, g0, e0);
    if (two) adamw_update<sizeof(G) == 2, W, EMA>(p, pb, m, v, ema, j * W, clip, lr1, b1, b2, eps, wd1, bc1, bc2_sqrt, d, omd, p1, m1, v1, g1, e1);
    const int64_t ni = i + 2 * stride;
    if (ni < lanes) load(ni, p0, m0, v0, g0, e0);
    if (ni + stride < lanes) load(ni + stride, p1, m1, v1, g1, e1);
  }
}

// What an entry point asks of adamw_launch.
struct AdamwEntry {
  const char* who;      // the entry family, as a refused call's error text names it
  bool table;           // bounds / group_of / n_ranges are given and needed
  bool ema;             // ema / ema_decay are given and needed (fp32 gradients only)
  bool any_shape;       // vlb_adamw_step: any n > 0 and element-aligned pointers are served, one element per lane when need be
};

// The host side of all six entry points; G = float | bf16.  Every check precedes the launch.
template <typename G>
static int adamw_launch(const AdamwEntry& en, float* master, void* param_bf16, const G* grad, float* m, float* v, float* ema, int64_t n,
                        const int64_t* bounds, const int32_t* group_of, int n_ranges, const float* lr, const float* weight_decay,
                        int n_groups, float beta1, float beta2, float eps, int step, const float* sumsq, float max_norm, float ema_decay,
                        void* stream) {
  constexpr bool F32 = sizeof(G) == 4;
  const bool vec = n % 8 == 0 && (((uintptr_t)master | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) % 16) == 0 &&
                   ((uintptr_t)grad % (4 * sizeof(G))) == 0 && ((uintptr_t)param_bf16 % 8) == 0;
  VLB_REQUIRE(n > 0 && (en.any_shape || n % 8 == 0) && master && grad && m && v && (ema || !en.ema) && step >= 1,
              en.any_shape ? "%s: bad args" : "%s: n must be a positive multiple of 8", en.who);
  VLB_REQUIRE(!en.ema || (F32 && ema_decay >= 0.f && ema_decay < 1.f), "%s: 0 <= ema_decay < 1 is needed", en.who);
  VLB_REQUIRE(lr && weight_decay && n_groups >= 1 && n_groups <= kAdamwMaxGroups, "%s: 1 <= n_groups <= 8 with their rates are needed",
              en.who);
  VLB_REQUIRE(!en.table || (bounds && group_of && n_ranges >= 1 && (int64_t)n_ranges <= n / 8 && ((uintptr_t)bounds % 8) == 0 &&
                            ((uintptr_t)group_of % 4) == 0),
              "%s: 1 <= n_ranges <= n / 8 with both tables (8- / 4-byte aligned) is needed", en.who);
  VLB_REQUIRE(vec || en.any_shape, "%s: buffers must be 16-byte (fp32) / 8-byte (bf16) aligned", en.who);
  AdamwGroupRates rates;
  for (int k = 0; k < kAdamwMaxGroups; ++k) {          // unused slots repeat group 0: a stray group index stays harmless
    rates.lr[k] = lr[k < n_groups ? k : 0];
    rates.wd[k] = weight_decay[k < n_groups ? k : 0];
  }
  const float bc1 = 1.f - powf(beta1, (float)step);
  const float bc2s = sqrtf(1.f - powf(beta2, (float)step));
  const AdamwTable table = !en.table ? kAdamwNoTable : n_ranges <= kAdamwLdsRanges ? kAdamwLdsTable : kAdamwGlobalTable;
  void (*kernel)(float*, bf16*, const G*, float*, float*, int64_t, const int64_t*, const int32_t*, int, AdamwGroupRates, float, float,
                 float, float, float, const float*, float, float*, float) = nullptr;
  if (!en.ema)
    kernel = table == kAdamwNoTable ? adamw_kernel<G, 4, kAdamwNoTable, false>
             : table == kAdamwLdsTable ? adamw_kernel<G, 4, kAdamwLdsTable, false> : adamw_kernel<G, 4, kAdamwGlobalTable, false>;
  if constexpr (F32) {
    if (en.ema)
      kernel = table == kAdamwNoTable ? adamw_kernel<G, 4, kAdamwNoTable, true>
               : table == kAdamwLdsTable ? adamw_kernel<G, 4, kAdamwLdsTable, true> : adamw_kernel<G, 4, kAdamwGlobalTable, true>;
    if (!vec) kernel = adamw_kernel<G, 1, kAdamwNoTable, false>;        // (any_shape: no table, no EMA)
  }
  const int64_t lanes = vec ? n / 4 : n;
  int64_t nb = (lanes + 511) / 512; if (nb > 32768) nb = 32768;
  hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(256), 0, as_stream(stream), master, (bf16*)param_bf16, grad, m, v, lanes, bounds,
                     group_of, n_ranges, rates, beta1, beta2, eps, bc1, bc2s, sumsq, max_norm, ema, ema_decay);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

}  // namespace

extern "C" int vlb_adamw_step(float* master, void* param_bf16, const float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                              float beta2, float eps, float weight_decay, int step, const float* sumsq, float max_norm, void* stream) {
  return adamw_launch<float>({"adamw", false, false, true}, master, param_bf16, grad, m, v, nullptr, n, nullptr, nullptr, 0, &lr,
                             &weight_decay, 1, beta1, beta2, eps, step, sumsq, max_norm, 0.f, stream);
}
extern "C" int vlb_adamw_step_g16(float* master, void* param_bf16, const void* grad_bf16, float* m, float* v, int64_t n, float lr,
                                  float beta1, float beta2, float eps, float weight_decay, int step, const float* sumsq, float max_norm,
                                  void* stream) {
  return adamw_launch<bf16>({"adamw_g16", false, false, false}, master, param_bf16, (const bf16*)grad_bf16, m, v, nullptr, n, nullptr,
                            nullptr, 0, &lr, &weight_decay, 1, beta1, beta2, eps, step, sumsq, max_norm, 0.f, stream);
}
// one launch for a store whose ranges have their own lr / weight_decay
extern "C" int vlb_adamw_step_groups(float* master, void* param_bf16, const float* grad, float* m, float* v, int64_t n,
                                     const int64_t* bounds, const int32_t* group_of, int n_ranges, const float* lr,
                                     const float* weight_decay, int n_groups, float beta1, float beta2, float eps, int step,
                                     const float* sumsq, float max_norm, void* stream) {
  return adamw_launch<float>({"adamw_groups", true, false, false}, master, param_bf16, grad, m, v, nullptr, n, bounds, group_of, n_ranges,
                             lr, weight_decay, n_groups, beta1, beta2, eps, step, sumsq, max_norm, 0.f, stream);
}
extern "C" int vlb_adamw_step_groups_g16(float* master, void* param_bf16, const void* grad_bf16, float* m, float* v, int64_t n,
                                         const int64_t* bounds, const int32_t* group_of, int n_ranges, const float* lr,
                                         const float* weight_decay, int n_groups, float beta1, float beta2, float eps, int step,
                                         const float* sumsq, float max_norm, void* stream) {
  return adamw_launch<bf16>({"adamw_groups_g16", true, false, false}, master, param_bf16, (const bf16*)grad_bf16, m, v, nullptr, n, bounds,
                            group_of, n_ranges, lr, weight_decay, n_groups, beta1, beta2, eps, step, sumsq, max_norm, 0.f, stream);
}
// the fp32 steps with an exponential moving average of the masters kept in the same launch
extern "C" int vlb_adamw_step_ema(float* master, void* param_bf16, const float* grad, float* m, float* v, float* ema, int64_t n,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, int step, const float* sumsq,
                                  float max_norm, float ema_decay, void* stream) {
  return adamw_launch<float>({"adamw_ema", false, true, false}, master, param_bf16, grad, m, v, ema, n, nullptr, nullptr, 0, &lr,
                             &weight_decay, 1, beta1, beta2, eps, step, sumsq, max_norm, ema_decay, stream);
}
extern "C" int vlb_adamw_step_groups_ema(float* master, void* param_bf16, const float* grad, float* m, float* v, float* ema, int64_t n,
                                         const int64_t* bounds, const int32_t* group_of, int n_ranges, const float* lr,
                                         const float* weight_decay, int n_groups, float beta1, float beta2, float eps, int step,
                                         const float* sumsq, float max_norm, float ema_decay, void* stream) {
  return adamw_launch<float>({"adamw_groups_ema", true, true, false}, master, param_bf16, grad, m, v, ema, n, bounds, group_of, n_ranges,
                             lr, weight_decay, n_groups, beta1, beta2, eps, step, sumsq, max_norm, ema_decay, stream);
}
