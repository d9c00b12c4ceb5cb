// bf16 MFMA GEMMs for gfx950:  C[M,N] = act(A[M,K].W[N,K]^T + A2.W2^T + bias) + residual
//
// Kernels:
//  * gemm_pp_kernel<BM,BN,WM,WN,..>: 512 threads (8 waves in two ping-pong groups), BK=64, LDS-DMA staging
//    (global_load_lds_dwordx4, swizzle applied on the SOURCE address), double-buffered LDS,
//    v_mfma_f32_16x16x32_bf16, XCD-aware tile order.  Needs N % BN == 0, K % 64 == 0; any M.
//  * gemm_w4_kernel<..>: the same tiles with 4 waves of 128x128 (or 96x128 / 128x64) blocks, for long K.
//  * gemm_generic_kernel: 64x64 tile, bounds-checked register staging, any M/N, K % 8 == 0.
//
// MFMA operand roles are swapped on purpose (rows of the MFMA = output COLUMNS n, columns of the
// MFMA = output rows m): each lane then owns 4 consecutive n of one row m per 16x16 tile, so the
// epilogue packs 4 bf16 into one 8-byte store and bias/residual are 8-byte loads.
#include <type_traits>

#include "common.hpp"

namespace {

constexpr int BK = 64;           // K elements per LDS tile row (128 bytes)
constexpr int ROW_BYTES = BK * 2;

struct GemmArgs {
  const bf16* A;  const bf16* W;  bf16* C;
  const bf16* A2; const bf16* W2;
  const bf16* bias; const bf16* residual;
  int M, N, K, K2;
  int lda, ldw, ldc, ldr, lda2, ldw2;
  int act;
  int tiles_m, tiles_n;     // grid of PARENT tiles (BM x BN*split_n) the tile order is defined on
  int tile0;                // first parent tile of this launch (the launch covers [tile0, tile0 + grid/split_n))
  int split_n;              // a workgroup computes 1/split_n of a parent tile's columns (tail launches)
  int grid;                 // workgroups of this launch (host side only)
  // masked second pair (LoRA backward through dropout): C = A.W^T + keep(m,n)/(1-p) * (A2.W2^T), keep from the
  // counter hash of lora.hip (fast 32-bit path): bits(m, n) = lowbias32((m*(N/2) + n/2) ^ key), 16 bits per column
  uint32_t drop_thresh, drop_key; float drop_scale;
  // split-K tail launch: the tiles of a partial last wave are each cut into k_splits contiguous K ranges, one
  // workgroup per (split, tile); raw fp32 accumulators go to ws[split][tile][wave][i][j][lane][4] and
  // gemm_splitk_reduce_kernel sums the splits in a fixed order and applies the epilogue
  float* ws; int k_splits, tail_tiles;
  int order;                // tile order (see tile_coords / xcd_remap_pid)
  // SWIGLU_PAIR only: when set, the pre-activations are ALSO stored, de-interleaved, as [gate | up] rows of N columns
  // (what a LoRA / full backward needs) - vlb_gemm_swiglu_save
  bf16* aux; int ldaux;
  int reserved;             // unused; keeps `wide` at its offset, where the kernels' scalar loads of the arguments pair up as before
  int wide;                 // C (and aux) rows 16-byte aligned: required by the four-wave kernels, which store 16 bytes per lane (store_pair16)
};

// blockIdx -> (m0, n0).  The order is defined on the full parent grid, so a GEMM can be cut into several launches (full
// waves with 256x256 tiles + a partial last wave re-tiled 256x128 or split along K) at any tile index.  Product order
// (GemmArgs::order = 3): column bands of 8 tiles with the rows walked inside a band, so 32 consecutive tiles are 4 rows x
// 8 columns (the 32 workgroups resident on one XCD share 4 A + 8 W panels in its L2), and xcd_remap_pid deals every
// round of 256 tiles to the eight XCDs in chunks of 32: at any moment the whole chip sweeps the row panels of A against
// the SAME 8 W panels, so a W panel comes out of HBM once and A (48-77 MB here) is re-read from the Infinity Cache.
// Against contiguous per-XCD runs over bands of 4 row tiles (order 0: 8 XCDs in 8 different places, 96 distinct panels
// per round instead of ~40) the same kernel measured +2 % (LoRA batch) / +7 % (frozen batch) on gate/up, -1.5 % / -2.3 %
// on the whole step (tools/ab_step_variant.py).  Orders 0-7 exist for A/B in the tools build.  When A is the larger operand
// and too large for the Infinity Cache the host picks order 2 instead (row bands dealt across the XCDs; pick_order).
__device__ __forceinline__ void tile_coords(const GemmArgs& p, int pid, int sub, int BM, int BN, int& m0, int& n0) {
  int tm, tn;
  if (p.order & 4) {
    // super-bands of 16 columns walked in groups of 4 rows, each group as two 4 x 8 chunks: with the chunks of a round
    // dealt to the XCDs (order bit 1) a chip-wide round is a 16 x 16 block of tiles = 16 A + 16 W panels
    const int sbt = 16 * p.tiles_m;
    const int sb = pid / sbt, c0 = sb * 16;
    const int wd = min(p.tiles_n - c0, 16);
    int w = pid - sb * sbt;
    const int rg = w / (4 * wd);
    const int gsz = min(p.tiles_m - 4 * rg, 4);
    w -= rg * 4 * wd;
    const int h = w / (gsz * 8);
    const int cw = min(wd - 8 * h, 8);
    w -= h * gsz * 8;
    tm = 4 * rg + w / cw;
    tn = c0 + 8 * h + w % cw;
  } else if (p.order & 1) {
    // column bands of 8 tiles, rows walked inside a band: 32 consecutive tiles = 4 rows x 8 columns, and one chip-wide
    // round of 256 tiles sweeps (almost) every row panel of A against the same 8 W panels
    constexpr int GROUP_N = 8;
    const int band = GROUP_N * p.tiles_m;
    const int cb = pid / band, c0 = cb * GROUP_N;
    const int csz = min(p.tiles_n - c0, GROUP_N);
    const int w = pid - cb * band;
    tm = w / csz;
    tn = c0 + w % csz;
  } else {
    constexpr int GROUP_M = 4;
    const int band = GROUP_M * p.tiles_n;
    const int g0 = (pid / band) * GROUP_M;
    const int gsz = min(p.tiles_m - g0, GROUP_M);
    tm = g0 + (pid % band) % gsz;
    tn = (pid % band) / gsz;
  }
  m0 = tm * BM;
  n0 = (tn * p.split_n + sub) * BN;
}

// blocks b and b+8 run on the same XCD.  order bit 1 clear: each XCD gets one contiguous run of the launch's work items;
// set: every round of 256 work items is dealt out in chunks of 32 (XCD x takes items [32x, 32x+32) of the round), so the
// eight XCDs work on neighbouring tiles at the same time and share what they pull through the Infinity Cache.
__device__ __forceinline__ int xcd_remap_pid(int order) {
  const int nblk = gridDim.x, pid = blockIdx.x;
  const int x = pid & 7, j = pid >> 3;
  int base = 0, n = nblk, jj = j;
  if (order & 2) {
    const int T = nblk >> 8, t = j >> 5;
    if (t < T) return (t << 8) + (x << 5) + (j & 31);
    base = T << 8; n = nblk - base; jj = j - (T << 5);
  }
  const int q = n >> 3, r = n & 7;
  return base + (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + jj;
}

// returns the K split of this workgroup (0 unless the launch is a split-K tail)
__device__ __forceinline__ int map_tile(const GemmArgs& p, int BM, int BN, int& m0, int& n0) {
  int pid = xcd_remap_pid(p.order);
  int sub = 0, ks = 0;
  if (p.split_n > 1) { sub = pid % p.split_n; pid /= p.split_n; }
  if (p.k_splits > 1) { ks = pid / p.tail_tiles; pid -= ks * p.tail_tiles; }   // split-major: an XCD's run shares one K range
  tile_coords(p, pid + p.tile0, sub, BM, BN, m0, n0);
  return ks;
}

__device__ __forceinline__ float apply_act(float x, int act) {
  switch (act) {
    case VLB_ACT_QUICK_GELU: return quick_gelu_f(x);
    case VLB_ACT_GELU: return gelu_erf_f(x);
    case VLB_ACT_SILU: return silu_f(x);
    default: return x;
  }
}

// (store_pair16, the 16-byte epilogue store shared with gemm_fp8.hip, lives in common.hpp)
// SWIGLU_PAIR epilogue piece: g / u = four consecutive gate / up pre-activations of row m (fragments 2j and 2j+1 of the
// interleaved weight), n = their column in the N/2-wide output.  With p.aux the pre-activations are kept too.
__device__ __forceinline__ void store_swiglu4(const GemmArgs& p, const f32x4& g, const f32x4& u, int m, int n) {
  bf16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (bf16)(silu_f(g[e]) * u[e]);
  *reinterpret_cast<bf16x4*>(p.C + (int64_t)m * p.ldc + n) = o;
  if (p.aux) {
    bf16x4 gb, ub;
#pragma unroll
    for (int e = 0; e < 4; ++e) { gb[e] = (bf16)g[e]; ub[e] = (bf16)u[e]; }
    bf16* ap = p.aux + (int64_t)m * p.ldaux + n;
    *reinterpret_cast<bf16x4*>(ap) = gb;
    *reinterpret_cast<bf16x4*>(ap + (p.N >> 1)) = ub;
  }
}

// two adjacent output fragments of the SWIGLU_PAIR epilogue (accumulator fragments 4q..4q+3) with 16-byte stores
__device__ __forceinline__ void store_swiglu8(const GemmArgs& p, const f32x4& g0, const f32x4& u0, const f32x4& g1, const f32x4& u1,
                                              int m, int n, int fq) {
  bf16x4 h0, h1;
#pragma unroll
  for (int e = 0; e < 4; ++e) { h0[e] = (bf16)(silu_f(g0[e]) * u0[e]); h1[e] = (bf16)(silu_f(g1[e]) * u1[e]); }
  store_pair16(p.C + (int64_t)m * p.ldc, n, h0, h1, fq);
  if (p.aux) {
    bf16x4 ga, gb, ua, ub;
#pragma unroll
    for (int e = 0; e < 4; ++e) { ga[e] = (bf16)g0[e]; gb[e] = (bf16)g1[e]; ua[e] = (bf16)u0[e]; ub[e] = (bf16)u1[e]; }
    bf16* ap = p.aux + (int64_t)m * p.ldaux;
    store_pair16(ap, n, ga, gb, fq);
    store_pair16(ap + (p.N >> 1), n, ua, ub, fq);
  }
}

// bias / activation / residual of one fragment piece: lane holds C[m][n .. n+3]
// ACT is a compile-time parameter: every fully unrolled epilogue nest then holds the code of ONE activation (see the
// instruction-cache note at w4_store_frag2); bias and residual stay run-time tests (a load and an add each).
template <int ACT>
__device__ __forceinline__ float act_apply(float x) {
  if constexpr (ACT == VLB_ACT_QUICK_GELU) return quick_gelu_f(x);
  else if constexpr (ACT == VLB_ACT_GELU) return gelu_erf_f(x);
  else if constexpr (ACT == VLB_ACT_SILU) return silu_f(x);
  else return x;
}
template <int ACT>
__device__ __forceinline__ bf16x4 w4_frag_value(const GemmArgs& p, f32x4 v, int m, int n) {
  if (p.bias) {
    const bf16x4 bb = *reinterpret_cast<const bf16x4*>(p.bias + n);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += (float)bb[e];
  }
  if constexpr (ACT != VLB_ACT_NONE) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = act_apply<ACT>(v[e]);
  }
  if (p.residual) {
    const bf16x4 rr = *reinterpret_cast<const bf16x4*>(p.residual + (int64_t)m * p.ldr + n);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += (float)rr[e];
  }
  bf16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (bf16)v[e];
  return o;
}
// run `BODY(ACT)` with the launch's activation as a compile-time constant (uniform dispatch, one nest executes)
#define VLB_DISPATCH_ACT(act, BODY)                        \
  do {                                                     \
    if ((act) == VLB_ACT_QUICK_GELU) { BODY(VLB_ACT_QUICK_GELU) } \
    else if ((act) == VLB_ACT_GELU) { BODY(VLB_ACT_GELU) }        \
    else if ((act) == VLB_ACT_SILU) { BODY(VLB_ACT_SILU) }        \
    else { BODY(VLB_ACT_NONE) }                                   \
  } while (0)

// LDS image of a [rows][64] bf16 tile: 128-byte rows, 16-byte chunk c of row r lives at slot
// c ^ ((r>>1)&7).  Two rows share one 256-byte bank row, so the 16 rows x 1 chunk column that a
// ds_read_b128 lane group touches land on 16 distinct 16-byte slots: conflict-free.
__device__ __forceinline__ int lds_off(int r, int c) { return r * ROW_BYTES + ((c ^ ((r >> 1) & 7)) << 4); }

// ------------------------------------------------------------------------------------------------
// Ping-pong 8-wave tile kernel.  The 8 waves form two groups of 4 (one wave of each group per
// SIMD).  Every K-tile is two phases (k-steps of 32); a phase is a LOAD segment (12 ds_read_b128 of
// fragments, plus the LDS-DMA issue of the tile after next) and a COMPUTE segment (32 MFMAs), separated
// by workgroup barriers.  Group 1 runs one barrier interval behind group 0, so on every SIMD one wave
// is always in its MFMA segment while its partner reads LDS: the matrix pipe never waits for loads.
//   interval:      0    1    2    3    4   ...
//   group 0:       L0   C0   L1   C1   L2  ...
//   group 1:       -    L0   C0   L1   C1  ...
// LDS-DMA for tile t+1 is issued in the first LOAD segment of tile t (its buffer was last read two
// intervals earlier, and every LOAD segment ends with lgkmcnt(0) before its barrier), and is waited for
// with ONE vmcnt(0) per tile placed just before the barrier that precedes the first read of tile t+1,
// i.e. after ~3-4 intervals of flight.
// ------------------------------------------------------------------------------------------------
// S0..S3: how many of the tile's LDS-DMA instructions a wave issues in load slot 0..3 of the 4-interval
// window that precedes the tile's first read (slot q of group 0 = its segments L0,C0,L1,C1 of tile t;
// of group 1 = C1 of tile t-1, then L0,C0,L1 of tile t).  S0+S1+S2+S3 = A_LD + B_LD.
// ABL (timing-only ablations, results are WRONG when non-zero): bit0 skip LDS-DMA in the loop, bit1 skip
// fragment reads in the loop, bit2 skip the barriers in the loop.
template <int BM, int BN, int WM, int WN, int S0, int S1, int S2, int S3, int ABL = 0>
__global__ __launch_bounds__(512, 2) void gemm_pp_kernel(GemmArgs p) {
  static_assert(WM * WN == 8 && WM % 2 == 0, "8 waves, groups split along M");
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int MT = TM / 16, NT = TN / 16;
  constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int A_LD = BM / 64, B_LD = BN / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  int m0, n0;
  map_tile(p, BM, BN, m0, n0);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int grp = wave >> 2;                       // 0: leads, 1: trails by one barrier interval

  const int srow = (lane >> 3), sslot = lane & 7;
  const bf16* a_src[A_LD]; const bf16* b_src[B_LD];
  const bf16* a2_src[A_LD]; const bf16* b2_src[B_LD];
#pragma unroll
  for (int i = 0; i < A_LD; ++i) {
    const int r = i * 64 + wave * 8 + srow;
    const int c = sslot ^ ((r >> 1) & 7);
    const int gm = min(m0 + r, p.M - 1);
    a_src[i] = p.A + (int64_t)gm * p.lda + c * 8;
    a2_src[i] = p.A2 ? p.A2 + (int64_t)gm * p.lda2 + c * 8 : nullptr;
  }
#pragma unroll
  for (int i = 0; i < B_LD; ++i) {
    const int r = i * 64 + wave * 8 + srow;
    const int c = sslot ^ ((r >> 1) & 7);
    b_src[i] = p.W + (int64_t)(n0 + r) * p.ldw + c * 8;
    b2_src[i] = p.W2 ? p.W2 + (int64_t)(n0 + r) * p.ldw2 + c * 8 : nullptr;
  }
  const int nk1 = p.K / BK;
  const int nk = nk1 + p.K2 / BK;

  static_assert(S0 + S1 + S2 + S3 == A_LD + B_LD, "slot counts must cover the tile");
  // instruction index i of a tile: 0..A_LD-1 = A pieces, A_LD.. = W pieces
  auto stage_range = [&](int buf, int kt, int from, int to) {
    char* base = smem + buf * STAGE + wave * 8 * ROW_BYTES;
    const bool first = kt < nk1;
    const int ko = (first ? kt : kt - nk1) * BK;
#pragma unroll
    for (int i = 0; i < A_LD + B_LD; ++i) {
      if (i < from || i >= to) continue;
      if (i < A_LD) glds16((first ? a_src[i] : a2_src[i]) + ko, base + i * 64 * ROW_BYTES);
      else glds16((first ? b_src[i - A_LD] : b2_src[i - A_LD]) + ko, base + A_BYTES + (i - A_LD) * 64 * ROW_BYTES);
    }
  };
  auto stage = [&](int buf, int kt) { stage_range(buf, kt, 0, A_LD + B_LD); };
  constexpr int O1 = S0, O2 = S0 + S1, O3 = S0 + S1 + S2, O4 = A_LD + B_LD;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  int a_off[MT][2], b_off[NT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) a_off[i][ks] = lds_off(wm * TM + i * 16 + fr, ks * 4 + fq);
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) b_off[j][ks] = A_BYTES + lds_off(wn * TN + j * 16 + fr, ks * 4 + fq);

#define PP_BARRIER()                                  \
  do {                                                \
    __builtin_amdgcn_sched_barrier(0);                \
    __builtin_amdgcn_s_barrier();                     \
    __builtin_amdgcn_sched_barrier(0);                \
  } while (0)
#define PP_LOOP_BARRIER()                             \
  do {                                                \
    if constexpr (!(ABL & 4)) { PP_BARRIER(); } else { __builtin_amdgcn_sched_barrier(0); } \
  } while (0)
#define PP_LGKM0() __builtin_amdgcn_s_waitcnt(0xc07f)
#define PP_VM0() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

  stage(0, 0);
  if (nk > 1) stage(1, 1);
  PP_VM0();
  PP_BARRIER();
  if (grp == 1) PP_BARRIER();

  bf16x8 af[MT], wf[NT];
  for (int kt = 0; kt < nk; ++kt) {
    const char* sb = smem + (kt & 1) * STAGE;
    const int nb = (kt & 1) ^ 1;                       // buffer of tile kt+1 (and of tile kt+2: kt&1)
    const bool ld1 = !(ABL & 1) && kt >= 1 && kt + 1 < nk;   // this window loads tile kt+1
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      // ---------------- LOAD segment
#pragma unroll
      for (int j = 0; j < NT; ++j) if ((ABL & 2) == 0 || kt == 0) wf[j] = *reinterpret_cast<const bf16x8*>(sb + b_off[j][ks]);
#pragma unroll
      for (int i = 0; i < MT; ++i) if ((ABL & 2) == 0 || kt == 0) af[i] = *reinterpret_cast<const bf16x8*>(sb + a_off[i][ks]);
      if (ld1) {
        if (grp == 0) { if (ks == 0) stage_range(nb, kt + 1, 0, O1); else stage_range(nb, kt + 1, O2, O3); }
        else          { if (ks == 0) stage_range(nb, kt + 1, O1, O2); else stage_range(nb, kt + 1, O3, O4); }
      }
      PP_LGKM0();
      if (ks == 1 && grp == 1 && kt >= 1) PP_VM0();
      PP_LOOP_BARRIER();
      // ---------------- COMPUTE segment
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      if (grp == 0) {
        if (ld1) { if (ks == 0) stage_range(nb, kt + 1, O1, O2); else stage_range(nb, kt + 1, O3, O4); }
      } else {
        if (ks == 0) { if (ld1) stage_range(nb, kt + 1, O2, O3); }
        else if (!(ABL & 1) && kt + 2 < nk) stage_range(kt & 1, kt + 2, 0, O1);   // slot 0 of the NEXT window
      }
      if (ks == 1 && grp == 0 && kt >= 1) PP_VM0();
      PP_LOOP_BARRIER();
    }
  }
  if (grp == 0) PP_BARRIER();
#undef PP_BARRIER
#undef PP_LOOP_BARRIER
#undef PP_LGKM0
#undef PP_VM0

  if (p.act == VLB_ACT_SWIGLU_PAIR) {
    // W rows are interleaved in 16-row blocks [gate_b | up_b]: n-tiles (2j, 2j+1) hold gate and up of the
    // same 16 output features at the same lane/register positions -> out = silu(gate) * up, N/2 columns.
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + wm * TM + i * 16 + fr;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < NT; j += 2) {
        store_swiglu4(p, acc[i][j], acc[i][j + 1], m, (n0 + wn * TN) / 2 + (j / 2) * 16 + fq * 4);
      }
    }
    return;
  }
  // C rows 16-byte aligned (p.wide): adjacent fragments paired into 16-byte stores (store_pair16); one nest per activation
#define PP_EPILOGUE_WIDE(ACT)                                                                                            \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                                                       \
    const int m = m0 + wm * TM + i * 16 + fr;                                                                            \
    if (m >= p.M) continue;                                                                                              \
    _Pragma("unroll") for (int j = 0; j < NT; j += 2) {                                                                  \
      const int n = n0 + wn * TN + j * 16 + fq * 4;                                                                      \
      store_pair16(p.C + (int64_t)m * p.ldc, n, w4_frag_value<ACT>(p, acc[i][j], m, n), w4_frag_value<ACT>(p, acc[i][j + 1], m, n + 16), fq); \
    }                                                                                                                    \
  }
#define PP_EPILOGUE_NARROW(ACT)                                                                                          \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                                                       \
    const int m = m0 + wm * TM + i * 16 + fr;                                                                            \
    if (m >= p.M) continue;                                                                                              \
    _Pragma("unroll") for (int j = 0; j < NT; ++j) {                                                                     \
      const int n = n0 + wn * TN + j * 16 + fq * 4;                                                                      \
      *reinterpret_cast<bf16x4*>(p.C + (int64_t)m * p.ldc + n) = w4_frag_value<ACT>(p, acc[i][j], m, n);                 \
    }                                                                                                                    \
  }
  if (p.wide) VLB_DISPATCH_ACT(p.act, PP_EPILOGUE_WIDE);
  else VLB_DISPATCH_ACT(p.act, PP_EPILOGUE_NARROW);
#undef PP_EPILOGUE_WIDE
#undef PP_EPILOGUE_NARROW
}

// ------------------------------------------------------------------------------------------------
// generic bounds-checked kernel: 64x64 tile, 256 threads (2x2 waves, each 32x32 = 2x2 MFMA tiles),
// BK = 32, register staging into padded LDS rows.  Correct for every shape with K % 8 == 0.
// ------------------------------------------------------------------------------------------------
constexpr int GK = 32;
constexpr int GLD = GK + 8;   // padded row (80 bytes): 16-byte aligned, breaks power-of-two stride

__global__ __launch_bounds__(256) void gemm_generic_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) bf16 sA[64 * GLD];
  __shared__ __attribute__((aligned(16))) bf16 sW[64 * GLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int fr = lane & 15, fq = lane >> 4;
  // each thread stages one 16-byte chunk of A and one of W per k-tile: row = tid/4, chunk = tid%4
  const int lr = tid >> 2, lc = tid & 3;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int pass = 0; pass < 2; ++pass) {
    const bf16* A = pass ? p.A2 : p.A;
    const bf16* W = pass ? p.W2 : p.W;
    const int K = pass ? p.K2 : p.K;
    const int lda = pass ? p.lda2 : p.lda, ldw = pass ? p.ldw2 : p.ldw;
    if (K == 0 || A == nullptr) continue;
    for (int k0 = 0; k0 < K; k0 += GK) {
      bf16x8 va = {}, vw = {};
      const int kk = k0 + lc * 8;
      if (m0 + lr < p.M && kk < K) va = *reinterpret_cast<const bf16x8*>(A + (int64_t)(m0 + lr) * lda + kk);
      if (n0 + lr < p.N && kk < K) vw = *reinterpret_cast<const bf16x8*>(W + (int64_t)(n0 + lr) * ldw + kk);
      __syncthreads();
      *reinterpret_cast<bf16x8*>(&sA[lr * GLD + lc * 8]) = va;
      *reinterpret_cast<bf16x8*>(&sW[lr * GLD + lc * 8]) = vw;
      __syncthreads();
      bf16x8 af[2], wf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const bf16x8*>(&sA[(wm * 32 + i * 16 + fr) * GLD + fq * 8]);
#pragma unroll
      for (int j = 0; j < 2; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(&sW[(wn * 32 + j * 16 + fr) * GLD + fq * 8]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
  }
  if (p.act == VLB_ACT_SWIGLU_PAIR) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + wm * 32 + i * 16 + fr;
      if (m >= p.M) continue;
      const int nb = (n0 + wn * 32) / 2 + fq * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (2 * (nb + e) < p.N) {
          p.C[(int64_t)m * p.ldc + nb + e] = (bf16)(silu_f(acc[i][0][e]) * acc[i][1][e]);
          if (p.aux) {
            p.aux[(int64_t)m * p.ldaux + nb + e] = (bf16)acc[i][0][e];
            p.aux[(int64_t)m * p.ldaux + (p.N >> 1) + nb + e] = (bf16)acc[i][1][e];
          }
        }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wm * 32 + i * 16 + fr;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int nb = n0 + wn * 32 + j * 16 + fq * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int n = nb + e;
        if (n >= p.N) continue;
        float v = acc[i][j][e];
        if (p.bias) v += (float)p.bias[n];
        v = apply_act(v, p.act);
        if (p.residual) v += (float)p.residual[(int64_t)m * p.ldr + n];
        p.C[(int64_t)m * p.ldc + n] = (bf16)v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Four-wave variant of the 256x256x64 tile: 256 threads = 2x2 waves, each wave owns a 128x128 block
// (8x8 MFMA tiles, 256 accumulator registers - one wave per SIMD with the full 512-register budget).
// Why: per K-tile the 8-wave kernels read (128+64)*64*2 B * 8 = 192 KB of fragments from LDS plus the
// 64 KB LDS-DMA write = 2048 LDS cycles at 128 B/clk - exactly the 2048 MFMA cycles of the tile, so the
// two pipes must overlap perfectly.  128x128 wave blocks read (128+128)*64*2 B * 4 = 128 KB (1536 cycles
// with the DMA): a quarter of the LDS time becomes slack, and one barrier per K-tile replaces four.
// Schedule of one wave (software pipelined, no partner wave to hide behind):
//   block 1:  MFMAs of k-step 0   || ds_reads of k-step 1 fragments
//   lgkmcnt(0), vmcnt(0) (tile t+1 landed; it was issued 1.5 tiles ago), s_barrier
//   block 2:  MFMAs of k-step 1   || LDS-DMA of tile t+2 into the buffer just released
//                                 || ds_reads of tile t+1's k-step 0 fragments
// Instruction mix per 4 MFMAs (64 cycles of matrix pipe): one ds_read_b128 (+ one LDS-DMA in block 2).
// ------------------------------------------------------------------------------------------------
// MFMA with the accumulator tied in place in an AGPR tuple.  With all 256 AGPRs holding accumulators the
// register allocator otherwise rotates destination tuples through copies; the asm form pins dst == srcC.
typedef int i32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void mfma_tied(f32x4& c, const bf16x8& a, const bf16x8& b) {
  asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0"
               : "+a"(c)
               : "v"(__builtin_bit_cast(i32x4_t, a)), "v"(__builtin_bit_cast(i32x4_t, b)));
}

// epilogue arithmetic of one 16x16 accumulator fragment: lane holds C[m][n .. n+3]
// SWIGLU_BWD: v = d(silu(gate)*up) for columns n..n+3 of a [M, N = ff] product; residual = the saved [gate | up] activations
// (row stride ldr), C = [d gate | d up] (row stride ldc): SwiGLU backward without materialising v
__device__ __forceinline__ void w4_swiglu_bwd_math(const f32x4& v, const bf16x4& g4, const bf16x4& u4, bf16x4& dg, bf16x4& du) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float g = (float)g4[e], u = (float)u4[e];
    const float sg = sigmoid_f(g);
    du[e] = (bf16)(v[e] * (g * sg));
    dg[e] = (bf16)(v[e] * u * (sg * (1.f + g * (1.f - sg))));
  }
}
// Two adjacent fragments (columns n.. and n+16..), 16-byte stores.  KIND picks ONE epilogue at compile time so that each
// kind's fully unrolled loop nest is a compact, contiguous instruction stream: with the kinds as run-time branches inside
// every fragment the executed path hopped over ~280 KB of never-executed activation code per tile - instruction-cache
// misses that cost the plain epilogue ~8 % of a whole K = 4096 GEMM (1.11 -> 1.03 ms on gate/up at the LoRA batch).
enum { EPI_PLAIN = 0, EPI_RESIDUAL = 1, EPI_SWIGLU_BWD = 2, EPI_GENERIC = 3 };     // EPI_GENERIC + act (0..3): bias / activation / residual
__device__ __forceinline__ bf16x4 cvt4(const f32x4& v) {
  bf16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = (bf16)v[e];
  return o;
}
template <int KIND>
__device__ __forceinline__ void w4_store_frag2(const GemmArgs& p, const f32x4& va, const f32x4& vb, int m, int n, int fq) {
  bf16* crow = p.C + (int64_t)m * p.ldc;
  if constexpr (KIND == EPI_SWIGLU_BWD) {
    // saved [gate | up] rows: one 16-byte load each for this lane's two fragment pieces (rows 16-byte aligned: host check)
    const bf16* grow = p.residual + (int64_t)m * p.ldr;
    bf16x4 ga, gb, ua, ub, dga, dua, dgb, dub;
    load_pair16(grow, n, fq, ga, gb);
    load_pair16(grow + p.N, n, fq, ua, ub);
    w4_swiglu_bwd_math(va, ga, ua, dga, dua);
    w4_swiglu_bwd_math(vb, gb, ub, dgb, dub);
    store_pair16(crow, n, dga, dgb, fq);
    store_pair16(crow + p.N, n, dua, dub, fq);
  } else if constexpr (KIND == EPI_PLAIN) {
    store_pair16(crow, n, cvt4(va), cvt4(vb), fq);
  } else if constexpr (KIND == EPI_RESIDUAL) {
    const bf16* rp = p.residual + (int64_t)m * p.ldr + n;
    const bf16x4 ra = *reinterpret_cast<const bf16x4*>(rp), rb = *reinterpret_cast<const bf16x4*>(rp + 16);
    f32x4 xa = va, xb = vb;
#pragma unroll
    for (int e = 0; e < 4; ++e) { xa[e] += (float)ra[e]; xb[e] += (float)rb[e]; }
    store_pair16(crow, n, cvt4(xa), cvt4(xb), fq);
  } else {       // EPI_GENERIC + ACT: KIND = EPI_GENERIC + the activation code
    constexpr int ACT = KIND - EPI_GENERIC;
    store_pair16(crow, n, w4_frag_value<ACT>(p, va, m, n), w4_frag_value<ACT>(p, vb, m, n + 16), fq);
  }
}
// which epilogue a launch needs (uniform): bias or an activation -> generic
__device__ __forceinline__ int w4_epilogue_kind(const GemmArgs& p) {
  if (p.act == VLB_ACT_SWIGLU_BWD) return EPI_SWIGLU_BWD;
  if (p.bias || p.act != VLB_ACT_NONE) return EPI_GENERIC;
  return p.residual ? EPI_RESIDUAL : EPI_PLAIN;
}
// NT = 8: 256x256 tile (wave block 128x128).  NT = 4: 256x128 tile (wave block 128x64) for the re-cut tiles
// of a partial last wave - same pipeline, 8 MFMA groups per block instead of 16.  MT = 6: 192-row tiles (wave
// block 96 rows), picked by the host when they quantise the row count into fewer, fuller waves of tiles.
// MASKED: the second operand pair (one K-tile, K2 = 64) runs FIRST, the accumulators are then multiplied by the
// dropout keep mask / (1-p) in place, and the main K loop continues on top - dx = dy.W + keep*(u.A)/(1-p) in one GEMM.
// ABL (timing-only ablations, tools build; results are WRONG when non-zero): bit0 skip the LDS-DMA of the loop, bit1 skip
// its fragment reads, bit2 skip its barrier, bit3 skip its vmcnt(0) wait, bit4 / bit5 stage W / A from panel 0 (L2-resident).
template <int NT = 8, int ABL = 0, int MT = 8, bool MASKED = false, bool SPLITK = false>
__global__ __launch_bounds__(256, 1) void gemm_w4_kernel(GemmArgs p) {
  constexpr int TM = 16 * MT, TN = 16 * NT, BM = 2 * TM, BN = 2 * TN;
  constexpr int NG = MT * NT / 4;                      // groups of 4 MFMAs per block (one k-step of the wave block)
  constexpr int LAST_A = NG / 2 + 1;                   // group in which the double-slotted last A fragment is fetched
  constexpr int A_BYTES = BM * ROW_BYTES, B_BYTES = BN * ROW_BYTES;
  constexpr int STAGE = A_BYTES + B_BYTES;
  constexpr int A_LD = BM / 32, B_LD = BN / 32;       // LDS-DMA instructions per thread per tile (32 rows each)
  constexpr int ND = A_LD + B_LD;
  static_assert((NT == 8 || NT == 4) && (MT == 8 || MT == 6), "wave block 128|96 rows x 128|64 columns");
  static_assert(ND <= 2 * NG && (NT - 1) < NG && (2 * (MT - 2) + 2) * NT / 8 < NG, "schedule does not fit the block");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  int m0, n0;
  const int nk1 = MASKED ? p.K2 / BK : p.K / BK;       // K-tiles of the pair that runs first
  const int nk_all = p.K / BK + p.K2 / BK;
  const int ksplit = map_tile(p, BM, BN, m0, n0);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // staging: instruction i of this wave fills LDS rows [i*32 + wave*8, +8) of A (i < A_LD) or W.
  // Sources are (uniform base) + 32-bit byte offset, recomputed per instruction from two row numbers:
  // no per-instruction pointer arrays (the 128 fragment + 256 accumulator registers leave no room).
  // The swizzle term ((r>>1)&7) is the same for rows r and r + 32*i.
  const int srow = (lane >> 3), sslot = lane & 7;
  const int r0 = wave * 8 + srow;
  const int colb = (sslot ^ ((r0 >> 1) & 7)) * 8;
  // (tools build, timing only: ABL bit 4 / 5 make every workgroup stage W / A panel 0 - operands that always hit in L2)
  const int rowA = (ABL & 32) ? r0 : m0 + r0, rowW = (ABL & 16) ? r0 : n0 + r0;
  // split-K tail: this workgroup walks K-tiles [kt_lo, kt_lo + nk) of the concatenated (pair 1 | pair 2) sequence
  const int kt_lo = SPLITK ? (int)((int64_t)ksplit * nk_all / p.k_splits) : 0;
  const int nk = SPLITK ? (int)((int64_t)(ksplit + 1) * nk_all / p.k_splits) - kt_lo : nk_all;

  // LDS-DMA sources = uniform base (SGPR pair, advanced 128 B per K-tile) + a per-instruction 32-bit
  // byte offset held in a VGPR: the loop issues each global_load_lds with no address arithmetic at all.
  // The offsets are rebuilt once when the K loop crosses into the second operand pair (A2, W2).
  uint32_t offA[A_LD], offW[B_LD];
  const char* curA; const char* curW;
  auto set_operands = [&](const bf16* A_, const bf16* W_, int lda_, int ldw_, int kt_in_pair) {
#pragma unroll
    for (int i = 0; i < A_LD; ++i)
      offA[i] = ((uint32_t)min(rowA + 32 * i, p.M - 1) * (uint32_t)lda_ + (uint32_t)colb) * 2u;
#pragma unroll
    for (int j = 0; j < B_LD; ++j) offW[j] = ((uint32_t)(rowW + 32 * j) * (uint32_t)ldw_ + (uint32_t)colb) * 2u;
    curA = reinterpret_cast<const char*>(A_) + (int64_t)kt_in_pair * ROW_BYTES;
    curW = reinterpret_cast<const char*>(W_) + (int64_t)kt_in_pair * ROW_BYTES;
  };
  auto select = [&](int rel) {          // call with consecutive rel = 0, 1, ..: positions the bases on K-tile kt_lo + rel
    const int kt = SPLITK ? rel + kt_lo : rel;
    if (rel == 0) {
      const bool second = SPLITK && kt >= nk1;
      if (MASKED != second) set_operands(p.A2, p.W2, p.lda2, p.ldw2, second ? kt - nk1 : kt);
      else set_operands(p.A, p.W, p.lda, p.ldw, second ? kt - nk1 : kt);
    }
    else if (kt == nk1) { if (MASKED) set_operands(p.A, p.W, p.lda, p.ldw, 0); else set_operands(p.A2, p.W2, p.lda2, p.ldw2, 0); }
    else { curA += ROW_BYTES; curW += ROW_BYTES; }
  };
  auto dma = [&](int buf, int i) {     // instruction i of the selected tile (0..A_LD-1: A, then W)
    char* base = smem + buf * STAGE + wave * 8 * ROW_BYTES;
    if (i < A_LD) glds16(curA + offA[i], base + i * 32 * ROW_BYTES);
    else glds16(curW + offW[i - A_LD], base + A_BYTES + (i - A_LD) * 32 * ROW_BYTES);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment offsets: tile i adds i*16 rows = i*2048 bytes (the swizzle term does not depend on i)
  const int fr = lane & 15, fq = lane >> 4;
  int a_off[2], b_off[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    a_off[ks] = lds_off(wm * TM + fr, ks * 4 + fq);
    b_off[ks] = A_BYTES + lds_off(wn * TN + fr, ks * 4 + fq);
  }
  auto frag = [&](const char* sb, int off, int t) { return *reinterpret_cast<const bf16x8*>(sb + off + t * 16 * ROW_BYTES); };

#define W4_FENCE() __builtin_amdgcn_sched_barrier(0)
#define W4_BARRIER() do { W4_FENCE(); __builtin_amdgcn_s_barrier(); W4_FENCE(); } while (0)

  select(0);
#pragma unroll
  for (int i = 0; i < A_LD + B_LD; ++i) dma(0, i);
  if (nk > 1) {
    select(1);
#pragma unroll
    for (int i = 0; i < A_LD + B_LD; ++i) dma(1, i);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(ND) : "memory");      // tile 0 landed; tile 1 (ND younger loads) may still fly
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  W4_BARRIER();

  // Fragment registers: W fragments are double-buffered (wf[0], wf[1]); A fragments are refreshed IN
  // PLACE - with the i-major MFMA order af[i] dies after groups 2i and 2i+1, so the next k-step's af[i]
  // is loaded right behind it.  Only af[7] dies too late (it would have to be read after the barrier that
  // releases its buffer), so it alone has a second slot (a7[2]).
  bf16x8 wf[2][NT], af[MT - 1], a7[2];
#pragma unroll
  for (int j = 0; j < NT; ++j) wf[0][j] = frag(smem, b_off[0], j);
#pragma unroll
  for (int i = 0; i < MT - 1; ++i) af[i] = frag(smem, a_off[0], i);
  a7[0] = frag(smem, a_off[0], MT - 1);
  __builtin_amdgcn_s_waitcnt(0xc07f);        // so that no compiler-inserted wait lands inside the loop
  W4_FENCE();

  // one K-tile; MORE: a tile kt+1 exists (fetch its first fragments), LOAD2: tile kt+2 exists (LDS-DMA it)
  auto tile = [&](int kt, auto more_c, auto load2_c) __attribute__((always_inline)) {
    constexpr bool MORE = decltype(more_c)::value, LOAD2 = decltype(load2_c)::value;
    const int buf = kt & 1;
    const char* sb = smem + buf * STAGE;
    const char* sn = smem + (buf ^ 1) * STAGE;
    // ---------------- block 1: MFMA(k-step 0) || reads of k-step 1
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (!(ABL & 2) || kt == 0) {
        if (g < NT) wf[1][g] = frag(sb, b_off[1], g);
        // af[i] dies with MFMA i*NT + NT-1, i.e. in group (i*NT + NT-1)/4; it is refetched in the next group
        if (g >= 1 && (g * 4) % NT == 0 && g * 4 / NT - 1 <= MT - 2) af[g * 4 / NT - 1] = frag(sb, a_off[1], g * 4 / NT - 1);
        if (g == LAST_A) a7[1] = frag(sb, a_off[1], MT - 1);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = g * 4 + q, i = t / NT, j = t % NT;
        mfma_tied(acc[i][j], wf[0][j], i == MT - 1 ? a7[0] : af[i]);
      }
      W4_FENCE();
    }
    // every wave is done reading buffer kt&1 (lgkmcnt) and its pieces of tile kt+1 have landed (vmcnt)
    __builtin_amdgcn_s_waitcnt(0xc07f);
    if constexpr (!(ABL & 8)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (!(ABL & 4)) { W4_BARRIER(); } else { W4_FENCE(); }
    if constexpr (LOAD2) select(kt + 2);
    // ---------------- block 2: MFMA(k-step 1) || DMA of tile kt+2 || reads of tile kt+1, k-step 0
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if constexpr (LOAD2 && !(ABL & 1)) {
        dma(buf, g);
        if (g + NG < ND) dma(buf, g + NG);
      }
      if constexpr (MORE && !(ABL & 2)) {
        if (g < NT) wf[0][g] = frag(sn, b_off[0], g);
        if (g >= 1 && (g * 4) % NT == 0 && g * 4 / NT - 1 <= MT - 2) af[g * 4 / NT - 1] = frag(sn, a_off[0], g * 4 / NT - 1);
        if (g == LAST_A) a7[0] = frag(sn, a_off[0], MT - 1);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = g * 4 + q, i = t / NT, j = t % NT;
        mfma_tied(acc[i][j], wf[1][j], i == MT - 1 ? a7[1] : af[i]);
      }
      W4_FENCE();
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);      // all of the next block's fragments are in (issued >= 2 groups ago)
    // accumulator copies the register allocator may place on the loop's exit edges must not overtake the
    // last (asm, hence opaque) MFMAs: XDL-write -> VALU-read needs up to 18 wait states
    asm volatile("s_nop 15" ::: "memory");
    W4_FENCE();
  };
  using T_ = std::true_type; using F_ = std::false_type;
  int kt = 0;
  if constexpr (MASKED) {
    // K-tile 0 = the LoRA pair u.A (host guarantees K2 == 64 and nk >= 3); then keep/(1-p) on the accumulators.
    // In a split-K tail only the first K range holds the pair: the others run their first main tile here and the
    // mask degenerates to keep-all x 1.0 (same straight-line code, no branch around the pinned accumulators).
    const bool later_range = SPLITK && ksplit != 0;
    const uint32_t m_thresh = later_range ? 0u : p.drop_thresh;
    const float m_scale = later_range ? 1.f : p.drop_scale;
    tile(0, T_{}, T_{});
    kt = 1;
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; j += 4)
        asm volatile("" : "+a"(acc[i][j]), "+a"(acc[i][j + 1]), "+a"(acc[i][j + 2]), "+a"(acc[i][j + 3]));
    const int frm = lane & 15, fqm = lane >> 4;
    const uint32_t halfN = (uint32_t)(p.N >> 1);
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const uint32_t rb = (uint32_t)(m0 + wm * TM + i * 16 + frm) * halfN;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const uint32_t pair0 = (uint32_t)(n0 + wn * TN + j * 16 + fqm * 4) >> 1;
        f32x4 v = acc[i][j];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          uint32_t h = (rb + pair0 + q) ^ p.drop_key;
          VLB_LOWBIAS32_STEPS(h);
          v[2 * q] = (h & 0xffffu) >= m_thresh ? v[2 * q] * m_scale : 0.f;
          v[2 * q + 1] = (h >> 16) >= m_thresh ? v[2 * q + 1] * m_scale : 0.f;
        }
        acc[i][j] = v;
        // straight back into its AGPR tuple, one tile at a time: keeps the VGPR live set (fragments of the next
        // K-tile are already in flight) small and the allocator from parking accumulators in VGPRs
        asm volatile("" : "+a"(acc[i][j]));
        W4_FENCE();
      }
    }
    asm volatile("s_nop 7" ::: "memory");          // VALU writes of the accumulators settle before the next MFMA reads them
  }
  for (; kt + 2 < nk; ++kt) tile(kt, T_{}, T_{});
  if (kt + 1 < nk) { tile(kt, T_{}, F_{}); ++kt; }
  tile(kt, F_{}, F_{});
  // The compiler does not know the asm statements are MFMAs: left alone it reads accumulators
  // (v_accvgpr_read for the epilogue) one cycle after the MFMA that produces them.  Re-define every
  // accumulator tile in (empty) asm statements placed after the wait, so all reads are ordered behind it.
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; j += 4)
      asm volatile("" : "+a"(acc[i][j]), "+a"(acc[i][j + 1]), "+a"(acc[i][j + 2]), "+a"(acc[i][j + 3]));
#undef W4_FENCE
#undef W4_BARRIER

  if constexpr (SPLITK) {
    // work item (= remapped block id) ksplit * tail_tiles + tile owns one [4 waves][MT][NT][64 lanes][4] slab
    float* wt = p.ws + ((int64_t)xcd_remap_pid(p.order) * 4 + wave) * (MT * NT * 256);
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
        *reinterpret_cast<f32x4*>(wt + ((i * NT + j) * 64 + lane) * 4) = acc[i][j];
    return;
  }
  // The four-wave kernels store 16 bytes per lane (store_pair16): the host only routes launches here whose C / aux rows are
  // 16-byte aligned (GemmArgs::wide).  One loop nest per epilogue kind - every loop over acc[][] must unroll completely
  // (a dynamically indexed accumulator array is moved to scratch memory, and with it the whole K loop).
  if (p.act == VLB_ACT_SWIGLU_PAIR) {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + wm * TM + i * 16 + fr;
      if (m >= p.M) continue;
#pragma unroll
      for (int j = 0; j < NT; j += 4)
        store_swiglu8(p, acc[i][j], acc[i][j + 1], acc[i][j + 2], acc[i][j + 3], m, (n0 + wn * TN) / 2 + (j / 2) * 16 + fq * 4, fq);
    }
    return;
  }
#define W4_EPILOGUE(KIND)                                                                                              \
  _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                                                      \
    const int m = m0 + wm * TM + i * 16 + fr;                                                                           \
    if (m >= p.M) continue;                                                                                             \
    _Pragma("unroll") for (int j = 0; j < NT; j += 2)                                                                   \
      w4_store_frag2<KIND>(p, acc[i][j], acc[i][j + 1], m, n0 + wn * TN + j * 16 + fq * 4, fq);                         \
  }
  const int kind = w4_epilogue_kind(p);
  if (kind == EPI_PLAIN) { W4_EPILOGUE(EPI_PLAIN) return; }
  if (kind == EPI_RESIDUAL) { W4_EPILOGUE(EPI_RESIDUAL) return; }
  if (kind == EPI_SWIGLU_BWD) { W4_EPILOGUE(EPI_SWIGLU_BWD) return; }
#define W4_EPILOGUE_ACT(ACT) W4_EPILOGUE(EPI_GENERIC + ACT)
  VLB_DISPATCH_ACT(p.act, W4_EPILOGUE_ACT);
#undef W4_EPILOGUE_ACT
#undef W4_EPILOGUE
}

// Second half of a split-K tail: block (tile, i) sums row-tile i of every wave's accumulators over the splits in
// a fixed order (deterministic) and applies the four-wave kernel's epilogue with the same thread <-> element map.
template <int MT, int NT>
__global__ __launch_bounds__(256) void gemm_splitk_reduce_kernel(GemmArgs p) {
  constexpr int TM = 16 * MT, TN = 16 * NT, BM = 2 * TM, BN = 2 * TN;
  const int tl = blockIdx.x / MT, i = blockIdx.x % MT;
  int m0, n0;
  tile_coords(p, p.tile0 + tl, 0, BM, BN, m0, n0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1, fr = lane & 15, fq = lane >> 4;
  f32x4 v[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < p.k_splits; ++s) {
    const float* wt = p.ws + ((int64_t)(s * p.tail_tiles + tl) * 4 + wave) * (MT * NT * 256);
#pragma unroll
    for (int j = 0; j < NT; ++j) v[j] += *reinterpret_cast<const f32x4*>(wt + ((i * NT + j) * 64 + lane) * 4);
  }
  const int m = m0 + wm * TM + i * 16 + fr;
  if (m >= p.M) return;
  if (p.act == VLB_ACT_SWIGLU_PAIR) {
#pragma unroll
    for (int j = 0; j < NT; j += 4) store_swiglu8(p, v[j], v[j + 1], v[j + 2], v[j + 3], m, (n0 + wn * TN) / 2 + (j / 2) * 16 + fq * 4, fq);
    return;
  }
  const int kind = w4_epilogue_kind(p);
#define W4_REDUCE_EPILOGUE(KIND) \
  _Pragma("unroll") for (int j = 0; j < NT; j += 2) w4_store_frag2<KIND>(p, v[j], v[j + 1], m, n0 + wn * TN + j * 16 + fq * 4, fq);
  if (kind == EPI_PLAIN) { W4_REDUCE_EPILOGUE(EPI_PLAIN) return; }
  if (kind == EPI_RESIDUAL) { W4_REDUCE_EPILOGUE(EPI_RESIDUAL) return; }
  if (kind == EPI_SWIGLU_BWD) { W4_REDUCE_EPILOGUE(EPI_SWIGLU_BWD) return; }
#define W4_REDUCE_EPILOGUE_ACT(ACT) W4_REDUCE_EPILOGUE(EPI_GENERIC + ACT)
  VLB_DISPATCH_ACT(p.act, W4_REDUCE_EPILOGUE_ACT);
#undef W4_REDUCE_EPILOGUE_ACT
#undef W4_REDUCE_EPILOGUE
}

template <int NT, int ABL, int MT = 8, bool MASKED = false, bool SPLITK = false>
int launch_w4(GemmArgs& a, hipStream_t s) {
  constexpr int LDS = 2 * (32 * MT + 32 * NT) * ROW_BYTES;
  // once per process and kernel; a function-local static's initialisation is thread-safe (C++11)
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_w4_kernel<NT, ABL, MT, MASKED, SPLITK>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
  if (attr != hipSuccess) {
    vlb_set_error("gemm: cannot reserve %d bytes of LDS: %s", LDS, hipGetErrorString(attr));
    return VLB_ERR_LAUNCH;
  }
  hipLaunchKernelGGL((gemm_w4_kernel<NT, ABL, MT, MASKED, SPLITK>), dim3(a.grid), dim3(256), LDS, s, a);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// partial last wave as a split-K pair of launches: a = the launch of the tail's parent tiles (tile0, tail_tiles,
// k_splits, ws set by the caller)
template <int MT, bool MASKED = false>
int launch_w4_splitk(GemmArgs& a, hipStream_t s) {
  a.split_n = 1;
  a.grid = a.k_splits * a.tail_tiles;
  int rc = launch_w4<8, 0, MT, MASKED, true>(a, s);
  if (rc != VLB_OK) return rc;
  hipLaunchKernelGGL((gemm_splitk_reduce_kernel<MT, 8>), dim3(a.tail_tiles * MT), dim3(256), 0, s, a);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// Kernel selection.  The product library (libvlb.so) is built WITHOUT VLB_TOOLS: the switches below are
// compile-time constants, no ablation is instantiated and no switch is exported.
// `make tools` builds libvlb_tools.so with -DVLB_TOOLS for tools/bench_gemm_variants.py & co: timing-only ablations of
// the product kernels (results wrong by construction) and switches that force one of the planner's or the router's
// own choices; nothing under phantom_vlb_amd/, bench.py or tests/ loads it.
#ifdef VLB_TOOLS
#define VLB_TUNABLE
constexpr bool kTools = true;
int g_variant = 3, g_force_tile = 0;      // kernel variant (3: the product's routing) and forced tile (0: none), see tools_override
#else
#define VLB_TUNABLE constexpr
constexpr bool kTools = false;
#endif
VLB_TUNABLE int g_tail_split = 1;   // split a mostly idle last wave of tiles into 256x128 tiles
VLB_TUNABLE int g_tile_order = 3;   // GemmArgs::order: bit 0 column bands of 8, bit 1 XCD chunks dealt per round, bit 2 16x16 rounds (A/B: variant bits 10-12 XOR 3)
VLB_TUNABLE int g_order_auto = 1;   // pick_order's shape rule (A/B: variant bit 13 disables it)
VLB_TUNABLE int g_tail_splitk = 1;  // ... or, when the caller passes a workspace, along K (A/B: variant bit 9 disables)
// Tile order for a shape.  The order decides which operand is swept once and which is re-read once per band, i.e. which
// one has to come back out of the 256 MB Infinity Cache: order 3 (column bands: W once, A re-read per band) unless A is the
// larger operand AND too large to stay cached (> 128 MB), then order 2 (row bands dealt across the XCDs: A once, W re-read).
// Measured (tools/bench_gemm_variants.py): gate/up at M = 5861 / 9447 / 15630 prefers 3 (+2 / +7 / +4 % over order 0), at
// M = 31260 (A = 256 MB) order 2 (+5 % over 3); `down` (K = 14336) at M >= 9447 (A >= 271 MB) order 2 (+2-4 %).
inline int pick_order(int M, int N, int K) {
  const double a_bytes = 2.0 * M * K, w_bytes = 2.0 * N * K;
  const int o = (a_bytes > w_bytes && a_bytes > 128e6) ? 2 : 3;
  return (g_tile_order == 3 && g_order_auto) ? o : g_tile_order;        // tools build: an explicit A/B order wins (variant bit 13: no shape rule)
}

// How the partial last wave of `tiles` tiles (nk K-tiles each) is run.  Costs are in units of one full wave of
// tiles: whole tiles 1.0; re-cut 256x128 halves 0.62 (measured 0.6-0.8); split-K 1/s plus ~16 K-tiles' worth
// (25-40 us measured) of fixed work (fp32 slab store, second launch, reduce).
struct TailPlan { int mode; int splits; double cost; };       // mode 0: none / whole tiles, 1: halves, 2: split-K
inline TailPlan plan_tail(int tiles, int nk, bool ws_ok, bool allow_halves = true) {
  const int cus = 256, r = tiles % cus;
  TailPlan t{0, 1, r == 0 ? 0.0 : 1.0};
  if (r == 0 || tiles <= cus) return t;
  if (allow_halves && g_tail_split && r <= cus * 5 / 8) t = TailPlan{1, 1, 0.62};
  if (ws_ok && g_tail_splitk) {
    int sp = cus / r; if (sp > 8) sp = 8;
    while (sp > 1 && nk / sp < 8) --sp;
    const double c = 1.0 / sp + 16.0 / nk;
    if (sp >= 2 && c < t.cost) t = TailPlan{2, sp, c};
  }
  return t;
}
// 192- or 256-row tiles for an [M, N] output (N % 256 == 0) on the four-wave kernel: cost = waves x tile rows, the
// smaller tile charged 2 % more; returns true for 192 rows.  Also hands back both tail plans.
inline bool plan_rows(int M, int N, int Ktot, bool ws_ok, TailPlan& p256, TailPlan& p192, bool splitk256 = true) {
  const int cus = 256, tn = N / 256, nk = Ktot / BK;
  const int tiles = ((M + 255) / 256) * tn, tiles192 = ((M + 191) / 192) * tn;
  p256 = plan_tail(tiles, nk, ws_ok && splitk256); p192 = plan_tail(tiles192, nk, ws_ok);
  const double c256 = (tiles / cus + p256.cost) * 256.0, c192 = (tiles192 / cus + p192.cost) * 192.0 * 1.02;
  return tiles > cus && c192 < 0.97 * c256;
}

template <int BM, int BN, int WM, int WN, int S0, int S1, int S2, int S3, int ABL = 0>
int launch_pp(GemmArgs& a, hipStream_t s, int lds) {
  // once per process and kernel; a function-local static's initialisation is thread-safe (C++11)
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_pp_kernel<BM, BN, WM, WN, S0, S1, S2, S3, ABL>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (attr != hipSuccess) {
    vlb_set_error("gemm: cannot reserve %d bytes of LDS: %s", lds, hipGetErrorString(attr));
    return VLB_ERR_LAUNCH;
  }
  hipLaunchKernelGGL((gemm_pp_kernel<BM, BN, WM, WN, S0, S1, S2, S3, ABL>), dim3(a.grid), dim3(512), lds, s, a);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// ------------------------------------------------------------------------------------------------
// Routing: plan_route states how one GEMM is cut into launches, run_route issues them; vlb_gemm_kernel_choice and
// vlb_gemm_plan export the same plan.
enum { FAM_GENERIC = 0, FAM_PP = 1, FAM_W4 = 2, FAM_NONE = 3 };     // generic 64x64 / ping-pong / four-wave kernel (NONE: tools build, unknown variant)
struct GemmRoute {
  int family;                 // kernel of the main launch
  int tail_family;            // ... of a column-halves tail launch (= family; the tools build can force them apart)
  int rows, cols;             // tile rows 256 | 192 (four-wave kernel only), tile columns 256 | 128
  int tiles_m, tiles_n;       // grid of parent tiles
  int main_tiles;             // parent tiles in the main launch (the full waves when there is a tail)
  int tail, tail_tiles;       // TailPlan::mode and the parent tiles of the partial last wave it covers
  int k_splits;               // K ranges per tail tile (tail mode 2)
  bool masked;                // the masked-pair kernels
  int abl;                    // 0; tools build: timing-only ablation of the main launch's kernel (results wrong by construction)
};
// What the routing depends on beyond the shape
struct RouteFacts {
  bool vec_ok;                // the tile kernels' pointer and stride rules hold (else: generic kernel)
  bool w4_ok;                 // the four-wave kernel may run: 16-byte stores (GemmArgs::wide) and 32-bit operand offsets (fits32)
  bool ws_ok;                 // the caller passed a split-K workspace
  bool w4_only;               // four-wave 256-column tiles are given (N % 256 == 0, K % 64 == 0): only the rows and the tail are planned
  bool masked;                // masked-pair rules: w4_only, the masked kernels, and no split-K at 256 rows
};
// the 4-wave kernel addresses operands with 32-bit byte offsets
inline bool fits32(int M, int N, int lda, int ldw, int lda2, int ldw2) {
  return (int64_t)M * lda < (1ll << 31) && (int64_t)N * ldw < (1ll << 31) && (int64_t)M * lda2 < (1ll << 31) && (int64_t)N * ldw2 < (1ll << 31);
}

// Cuts the output into tiles of r.cols columns for the kernel family already chosen: 192 or 256 rows (rows = 0: the
// cost model decides; 192 only on the four-wave kernel), full waves in the main launch, the partial last wave as planned.
//
// Tail split: when the 256x256 grid ends in a mostly idle last wave of tiles (e.g. 2576 tiles = 10.06
// waves for gate/up at M=5861), the full waves run as 256x256 tiles and the tiles of the partial wave
// are re-cut into 256x128 halves in a second launch, which spreads them over twice as many CUs for
// half as long.  Both launches walk the same tile order (map_tile), so the cut can be at any tile.
// Row quantisation: 192-row tiles (four-wave kernel only) when they cut the row count into fewer, fuller
// waves - e.g. M=5861, N=4096: 23x16 = 368 tiles of 256 rows cost (1 + 0.62 tail) x 256 = 415 row-units,
// 31x16 = 496 tiles of 192 rows cost 2 x 192 = 384.  Cost = waves x tile rows; a re-cut partial wave = 0.62.
inline void cut_waves(GemmRoute& r, int M, int N, int Ktot, bool ws_ok, bool splitk256, int rows = 0) {
  const bool w4 = r.family == FAM_W4;
  TailPlan p256{0, 1, 0.0}, p192 = p256;
  bool use192 = r.cols == 256 && plan_rows(M, N, Ktot, ws_ok && w4, p256, p192, splitk256) && w4;
  if (rows) use192 = rows == 192;
  const TailPlan& t = use192 ? p192 : p256;
  r.rows = use192 ? 192 : 256;
  r.tiles_m = (M + r.rows - 1) / r.rows; r.tiles_n = N / r.cols;
  r.tail = t.mode; r.k_splits = t.splits;
  r.tail_tiles = t.mode ? r.tiles_m * r.tiles_n % 256 : 0;
  r.main_tiles = r.tiles_m * r.tiles_n - r.tail_tiles;
}

// The launches of one GEMM.  Pure host arithmetic: no HIP call, nothing read but its arguments (and, in the tools
// build, the planner switches above).
inline GemmRoute plan_route(int M, int N, int K, int K2, const RouteFacts& f) {
  const int cus = 256;
  GemmRoute r{FAM_GENERIC, FAM_GENERIC, 64, 64, 0, 0, 0, 0, 0, 1, f.masked, 0};
  if (f.w4_only) {
    r.cols = 256;
  } else {
    if (!f.vec_ok || K % BK != 0 || K2 % BK != 0 || K == 0 || M < 128) return r;
    // the 256x256 tile has the better MFMA:LDS ratio; fall back to 256x128 only when the grid
    // would leave more than half of the chip idle
    if (N % 256 == 0) r.cols = ((M + 255) / 256) * (N / 256) < cus / 2 ? 128 : 256;
    else if (N % 128 == 0) r.cols = 128;
    else return r;
  }
  // the four-wave kernel wins once the K loop is long enough to amortise its serial prologue and epilogue (one
  // workgroup per CU, nothing to overlap them with): measured crossover K ~ 3072-4096
  r.family = r.tail_family = (f.w4_only || (f.w4_ok && K + K2 >= 4096)) ? FAM_W4 : FAM_PP;
  // (no split-K for the 256-row masked kernel: with 64 accumulator tiles + the mask temporaries the register
  // allocator starts rotating accumulator tuples behind the asm MFMAs; 192-row tiles are fine)
  cut_waves(r, M, N, K + K2, f.ws_ok, !f.masked);
  return r;
}

#ifdef VLB_TOOLS
// libvlb_tools.so only: vlb_gemm_set_variant's kernel variant (g_variant) and forced tile (g_force_tile) applied to the
// planned route.  (Its planner switches - variant bits 8-13 - act inside plan_tail and pick_order.)
//   variant 1: ping-pong kernel; 2: four-wave kernel whenever it may run (256x128 tiles: for long K); 3: the product's
//   choice; 4: like 3 without row planning, 8-wave kernel for the re-cut tail; 5: like 3 but always 192-row tiles for
//   long K; 6: like 3 but never 192-row tiles; 0x11-0x17 / 0x21-0x28 / 0x41-0x43 / 0x30-0x3b: ablations of the ping-pong
//   256x256 / four-wave 256-row (0x4n: W / A / both always from panel 0, L2-resident) / four-wave 192-row kernel
//   force_tile 1: 256x256 tiles, 2: 256x128 tiles (both: no row planning, no split-K); masked pair: 3 / 4 = 256- / 192-row tiles
inline void tools_override(GemmRoute& r, int M, int N, int K, int K2, const RouteFacts& f) {
  const int v = g_variant, ft = g_force_tile, Ktot = K + K2;
  if (f.masked) {
    if (ft == 3 || ft == 4) cut_waves(r, M, N, Ktot, f.ws_ok, false, ft == 3 ? 256 : 192);
    return;
  }
  if (r.family == FAM_GENERIC) return;
  if (ft == 1 && N % 256 == 0) r.cols = 256;
  if (ft == 2) r.cols = 128;
  const bool w4 = f.w4_ok && Ktot >= 4096, known = (v >= 1 && v <= 6) || v >= 0x10;
  r.tail_family = !known ? FAM_NONE : ((v == 2 || v == 3 || v == 5 || v == 6) && w4) ? FAM_W4 : FAM_PP;
  r.family = r.cols == 128 ? r.tail_family : FAM_W4;
  // the row planner and the split-K tail: variants 3, 5, 6 and the 192-row ablations, long K, no forced tile
  const bool planned = r.cols == 256 && (v == 3 || v == 5 || v == 6 || (v & 0xf0) == 0x30) && w4 && ft == 0;
  const bool multi_wave = ((M + 255) / 256) * (N / 256) > 256;
  cut_waves(r, M, N, Ktot, planned && f.ws_ok, true, !planned || v == 6 ? 256 : v == 3 ? 0 : multi_wave ? 192 : 256);
  if (r.cols == 128) return;
  if (r.rows == 192) {
    r.tail_family = FAM_W4;
    constexpr int abl192[16] = {0, 1, 2, 0, 4, 0, 0, 7, 8, 16, 32, 48, 0, 0, 0, 0};      // 0x39 / 0x3a / 0x3b: W / A / both always from panel 0
    if ((v & 0xf0) == 0x30) r.abl = abl192[v & 0xf];
    if (r.abl) r.tail = 0;          // whole-tile launches only
    return;
  }
  const int lo = v & 0xf;
  r.family = !known ? FAM_NONE : (v == 2 ? f.w4_ok : v <= 6 ? v >= 3 && w4 : false) ? FAM_W4 : FAM_PP;
  if ((v & 0xf0) == 0x10 && (lo == 1 || lo == 2 || lo == 3 || lo == 4 || lo == 6 || lo == 7)) r.abl = lo;
  if ((v & 0xf0) == 0x20 && (lo == 1 || lo == 2 || lo == 4 || lo == 7 || lo == 8) && f.w4_ok) { r.family = FAM_W4; r.abl = lo; }
  if (v >= 0x41 && v <= 0x43 && f.w4_ok) { r.family = FAM_W4; r.abl = 16 * (v & 3); }
}
#else
inline void tools_override(GemmRoute&, int, int, int, int, const RouteFacts&) {}
#endif

// Route -> kernel instantiation, the only place a tile kernel is named on the host.
constexpr int kernel_key(int family, int rows, int cols, bool masked = false, bool splitk = false, int abl = 0) {
  return family | (rows / 64) << 2 | (cols / 64) << 5 | masked << 8 | splitk << 9 | abl << 10;
}
template <bool TOOLS>
int launch_kernel(int key, GemmArgs& a, hipStream_t s) {
  constexpr int PP = FAM_PP, W4 = FAM_W4, T = TOOLS;
  switch (key) {
    case kernel_key(FAM_GENERIC, 64, 64):
      hipLaunchKernelGGL(gemm_generic_kernel, dim3((a.N + 63) / 64, (a.M + 63) / 64), dim3(256), 0, s, a);
      VLB_LAUNCH_CHECK();
      return VLB_OK;
    case kernel_key(PP, 256, 256): return launch_pp<256, 256, 2, 4, 8, 0, 0, 0>(a, s, 2 * (256 + 256) * ROW_BYTES);
    case kernel_key(PP, 256, 128): return launch_pp<256, 128, 4, 2, 6, 0, 0, 0>(a, s, 2 * (256 + 128) * ROW_BYTES);
    case kernel_key(W4, 256, 256): return launch_w4<8, 0, 8>(a, s);
    case kernel_key(W4, 256, 128): return launch_w4<4, 0, 8>(a, s);
    case kernel_key(W4, 192, 256): return launch_w4<8, 0, 6>(a, s);
    case kernel_key(W4, 192, 128): return launch_w4<4, 0, 6>(a, s);
    case kernel_key(W4, 256, 256, false, true): return launch_w4_splitk<8>(a, s);
    case kernel_key(W4, 192, 256, false, true): return launch_w4_splitk<6>(a, s);
    case kernel_key(W4, 256, 256, true): return launch_w4<8, 0, 8, true>(a, s);
    case kernel_key(W4, 256, 128, true): return launch_w4<4, 0, 8, true>(a, s);
    case kernel_key(W4, 192, 256, true): return launch_w4<8, 0, 6, true>(a, s);
    case kernel_key(W4, 192, 128, true): return launch_w4<4, 0, 6, true>(a, s);
    case kernel_key(W4, 192, 256, true, true): return launch_w4_splitk<6, true>(a, s);
  }
  if constexpr (TOOLS) {      // timing-only ablations of the main launch (ABL * T: instantiated in the tools build only)
    switch (key) {
#define VLB_ABL_PP(ABL) case kernel_key(PP, 256, 256, false, false, ABL): return launch_pp<256, 256, 2, 4, 8, 0, 0, 0, ABL * T>(a, s, 2 * (256 + 256) * ROW_BYTES);
#define VLB_ABL_W4(ABL)                                                                        \
  case kernel_key(W4, 256, 256, false, false, ABL): return launch_w4<8, ABL * T, 8>(a, s);      \
  case kernel_key(W4, 192, 256, false, false, ABL): return launch_w4<8, ABL * T, 6>(a, s);
      VLB_ABL_PP(1) VLB_ABL_PP(2) VLB_ABL_PP(3) VLB_ABL_PP(4) VLB_ABL_PP(6) VLB_ABL_PP(7)
      VLB_ABL_W4(1) VLB_ABL_W4(2) VLB_ABL_W4(4) VLB_ABL_W4(7) VLB_ABL_W4(8) VLB_ABL_W4(16) VLB_ABL_W4(32) VLB_ABL_W4(48)
#undef VLB_ABL_PP
#undef VLB_ABL_W4
    }
  }
  vlb_set_error("gemm: no kernel for this route (tools build: unknown kernel variant)");
  return VLB_ERR_INVALID;
}

// Issues a route: the main launch, then the partial last wave as column halves or as a split-K pair of launches.
inline int run_route(const GemmRoute& r, GemmArgs a, float* ws, hipStream_t s) {
  if (r.family == FAM_GENERIC) return launch_kernel<kTools>(kernel_key(FAM_GENERIC, 64, 64), a, s);
  a.tiles_m = r.tiles_m; a.tiles_n = r.tiles_n;
  a.grid = r.main_tiles;
  int rc = launch_kernel<kTools>(kernel_key(r.family, r.rows, r.cols, r.masked, false, r.abl), a, s);
  if (rc != VLB_OK || !r.tail) return rc;
  a.tile0 = r.main_tiles;
  if (r.tail == 2) {
    a.ws = ws; a.k_splits = r.k_splits; a.tail_tiles = r.tail_tiles;
    return launch_kernel<kTools>(kernel_key(FAM_W4, r.rows, 256, r.masked, true), a, s);
  }
  a.split_n = 2; a.grid = 2 * r.tail_tiles;
  return launch_kernel<kTools>(kernel_key(r.tail_family, r.rows, 128, r.masked), a, s);
}

// The kernels' argument block for one GEMM; the launch fields (tiles, tile0, grid, split-K) are run_route's.
inline GemmArgs gemm_args(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K, const void* bias,
                          const void* residual, int ldr, int act, const void* A2, int lda2, const void* W2, int ldw2, int K2,
                          void* aux, int ldaux) {
  GemmArgs a;
  a.A = (const bf16*)A; a.W = (const bf16*)W; a.C = (bf16*)C;
  a.A2 = (const bf16*)A2; a.W2 = (const bf16*)W2;
  a.bias = (const bf16*)bias; a.residual = (const bf16*)residual;
  a.M = M; a.N = N; a.K = K; a.K2 = K2;
  a.lda = lda; a.ldw = ldw; a.ldc = ldc; a.ldr = ldr; a.lda2 = lda2; a.ldw2 = ldw2;
  a.act = act; a.tiles_m = 0; a.tiles_n = 0; a.tile0 = 0; a.split_n = 1; a.grid = 0; a.drop_thresh = 0; a.drop_key = 0; a.drop_scale = 1.f;
  a.ws = nullptr; a.k_splits = 0; a.tail_tiles = 0; a.order = pick_order(M, N, K); a.aux = (bf16*)aux; a.ldaux = ldaux; a.reserved = 0;
  // ... and stores 16 bytes per lane (a.wide: C / aux rows 16-byte aligned)
  a.wide = ((uintptr_t)C % 16) == 0 && ldc % 8 == 0 && (!aux || (((uintptr_t)aux % 16) == 0 && ldaux % 8 == 0 && (N / 2) % 8 == 0));
  return a;
}

// 16x16 LDS-tiled transpose, 32x32 elements per block
__global__ void transpose_kernel(const bf16* __restrict__ in, bf16* __restrict__ out, int R, int C) {
  __shared__ bf16 t[32][33];
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  for (int i = threadIdx.y; i < 32; i += blockDim.y) {
    const int r = r0 + i, c = c0 + threadIdx.x;
    if (r < R && c < C) t[i][threadIdx.x] = in[(int64_t)r * C + c];
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += blockDim.y) {
    const int c = c0 + i, r = r0 + threadIdx.x;
    if (r < R && c < C) out[(int64_t)c * R + r] = t[threadIdx.x][i];
  }
}

}  // namespace

// The planner the dispatch runs (plan_route), for tests / DESIGN.md, with every alignment rule taken as met:
// the tile vlb_gemm_bf16 picks: 0 generic, 1 = 256x256, 2 = 256x128
extern "C" int vlb_gemm_kernel_choice(int M, int N, int K, int K2) {
  const GemmRoute r = plan_route(M, N, K, K2, RouteFacts{true, true, false, false, false});
  return r.family == FAM_GENERIC ? 0 : r.cols == 256 ? 1 : 2;
}

// ... and how a long-K GEMM on the four-wave kernel's 256-column tiles is cut: rows*1000 + tail mode*100 + K splits
// (tail mode 0 whole tiles, 1 re-cut halves, 2 split-K).
extern "C" int vlb_gemm_plan(int M, int N, int K, int K2, int with_workspace) {
  if (N % 256 != 0 || K + K2 < 4096) return 0;
  const GemmRoute r = plan_route(M, N, K, K2, RouteFacts{true, true, (with_workspace & 1) != 0, true, (with_workspace & 2) != 0});     // bit 1: masked-pair rules
  return r.rows * 1000 + r.tail * 100 + r.k_splits;
}

extern "C" int64_t vlb_gemm_workspace_bytes(void) { return 256ll * 256 * 256 * 4; }   // <= 256 work items x one 256x256 fp32 tile

static int gemm_impl(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                     const void* bias, const void* residual, int ldr, int act, const void* A2, int lda2,
                     const void* W2, int ldw2, int K2, void* ws, int64_t ws_bytes, void* stream, void* aux, int ldaux) {
  VLB_REQUIRE(A && W && C, "gemm: null operand");
  VLB_REQUIRE(!ws || ((uintptr_t)ws % 16) == 0, "gemm: workspace must be 16-byte aligned");
  const bool ws_ok = ws && ws_bytes >= vlb_gemm_workspace_bytes();
  VLB_REQUIRE(M > 0 && N > 0 && K > 0, "gemm: bad shape M=%d N=%d K=%d", M, N, K);
  VLB_REQUIRE(K % 8 == 0 && lda % 8 == 0 && ldw % 8 == 0, "gemm: K/lda/ldw must be multiples of 8 (K=%d lda=%d ldw=%d)", K, lda, ldw);
  VLB_REQUIRE(lda >= K && ldw >= K && (ldc >= N || (act == VLB_ACT_SWIGLU_PAIR && ldc >= N / 2)), "gemm: leading dimension smaller than row");
  if (K2 > 0) {
    VLB_REQUIRE(A2 && W2, "gemm: K2>0 needs A2 and W2");
    VLB_REQUIRE(K2 % 8 == 0 && lda2 % 8 == 0 && ldw2 % 8 == 0 && lda2 >= K2 && ldw2 >= K2, "gemm: bad second operand pair");
  } else {
    A2 = nullptr; W2 = nullptr; K2 = 0;
  }
  if (residual) VLB_REQUIRE(ldr >= N, "gemm: ldr < N");
  if (act == VLB_ACT_SWIGLU_PAIR) {
    VLB_REQUIRE(N % 32 == 0 && !bias && !residual && ldc >= N / 2, "gemm: SWIGLU_PAIR needs N %% 32 == 0, no bias/residual, ldc >= N/2");
  }
  const GemmArgs a = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, bias, residual, ldr, act, A2, lda2, W2, ldw2, K2, aux, ldaux);
  const bool vec_ok = (ldc % 4 == 0) && (!residual || ldr % 4 == 0) && (!aux || (ldaux % 4 == 0 && (N / 2) % 4 == 0)) &&
                      (((uintptr_t)C | (uintptr_t)residual | (uintptr_t)bias | (uintptr_t)aux) % 8 == 0) &&
                      (((uintptr_t)A | (uintptr_t)W | (uintptr_t)A2 | (uintptr_t)W2) % 16 == 0);
  const RouteFacts f{vec_ok, a.wide && fits32(M, N, lda, ldw, lda2, ldw2), ws_ok, false, false};
  GemmRoute r = plan_route(M, N, K, K2, f);
  tools_override(r, M, N, K, K2, f);      // empty in the product library
  return run_route(r, a, (float*)ws, as_stream(stream));
}

extern "C" int vlb_gemm_bf16(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                             const void* bias, const void* residual, int ldr, int act, const void* A2, int lda2,
                             const void* W2, int ldw2, int K2, void* stream) {
  return vlb_gemm_bf16_ws(A, lda, W, ldw, C, ldc, M, N, K, bias, residual, ldr, act, A2, lda2, W2, ldw2, K2, nullptr, 0, stream);
}

extern "C" int vlb_gemm_bf16_ws(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                                const void* bias, const void* residual, int ldr, int act, const void* A2, int lda2,
                                const void* W2, int ldw2, int K2, void* ws, int64_t ws_bytes, void* stream) {
  return gemm_impl(A, lda, W, ldw, C, ldc, M, N, K, bias, residual, ldr, act, A2, lda2, W2, ldw2, K2, ws, ws_bytes, stream, nullptr, 0);
}

extern "C" int vlb_gemm_swiglu_save(const void* A, int lda, const void* W_il, int ldw, void* H, int ldh, void* GU, int ldgu, int M, int N,
                                    int K, const void* A2, int lda2, const void* W2_il, int ldw2, int K2, void* ws, int64_t ws_bytes,
                                    void* stream) {
  VLB_REQUIRE(GU && ldgu >= N && ldgu % 4 == 0 && N % 8 == 0 && ((uintptr_t)GU % 8) == 0,
              "gemm_swiglu_save: [gate | up] rows must hold N columns, 8-byte aligned (N=%d ldgu=%d)", N, ldgu);
  return gemm_impl(A, lda, W_il, ldw, H, ldh, M, N, K, nullptr, nullptr, 0, VLB_ACT_SWIGLU_PAIR, A2, lda2, W2_il, ldw2, K2, ws, ws_bytes,
                   stream, GU, ldgu);
}

// Same wave-quantisation choice as vlb_gemm_bf16 (256- or 192-row tiles; partial wave re-cut or split along K), always on
// the four-wave kernel.
static int masked_pair_impl(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                            const void* A2, int lda2, const void* W2, int ldw2, float drop_p, uint32_t seed,
                            void* ws, int64_t ws_bytes, void* stream, int act, const void* residual, int ldr) {
  VLB_REQUIRE(!ws || ((uintptr_t)ws % 16) == 0, "gemm_masked_pair: workspace must be 16-byte aligned");
  const bool ws_ok = ws && ws_bytes >= vlb_gemm_workspace_bytes();
  VLB_REQUIRE(A && W && C && A2 && W2, "gemm_masked_pair: null operand");
  VLB_REQUIRE(M > 0 && N % 256 == 0 && K >= 128 && K % 64 == 0, "gemm_masked_pair: needs N %% 256 == 0, K %% 64 == 0, K >= 128 (N=%d K=%d)", N, K);
  VLB_REQUIRE(lda % 8 == 0 && ldw % 8 == 0 && lda2 % 8 == 0 && ldw2 % 8 == 0 && lda >= K && ldw >= K && lda2 >= 64 && ldw2 >= 64 &&
                  ldc % 4 == 0 && ldc >= N, "gemm_masked_pair: bad leading dimensions");
  VLB_REQUIRE((((uintptr_t)A | (uintptr_t)W | (uintptr_t)A2 | (uintptr_t)W2 | (uintptr_t)C) % 16) == 0 && ldc % 8 == 0,
              "gemm_masked_pair: operands and C rows must be 16-byte aligned");
  VLB_REQUIRE(drop_p > 0.f && drop_p < 1.f, "gemm_masked_pair: drop_p must be in (0,1) - use vlb_gemm_bf16 when p == 0");
  VLB_REQUIRE(fits32(M, N, lda, ldw, lda2, ldw2) && (int64_t)M * (N >> 1) < (1ll << 32),
              "gemm_masked_pair: operand too large for 32-bit offsets / the 32-bit dropout counter");
  GemmArgs a = gemm_args(A, lda, W, ldw, C, ldc, M, N, K, nullptr, residual, ldr, act, A2, lda2, W2, ldw2, 64, nullptr, 0);
  a.drop_thresh = thresh16(drop_p);
  a.drop_key = lowbias32(seed);
  a.drop_scale = 1.f / (1.f - drop_p);
  const RouteFacts f{true, true, ws_ok, true, true};
  GemmRoute r = plan_route(M, N, K, 64, f);
  tools_override(r, M, N, K, 64, f);      // empty in the product library
  return run_route(r, a, (float*)ws, as_stream(stream));
}

extern "C" int vlb_gemm_bf16_masked_pair(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                                         const void* A2, int lda2, const void* W2, int ldw2, float drop_p, uint32_t seed,
                                         void* stream) {
  return vlb_gemm_bf16_masked_pair_ws(A, lda, W, ldw, C, ldc, M, N, K, A2, lda2, W2, ldw2, drop_p, seed, nullptr, 0, stream);
}

extern "C" int vlb_gemm_bf16_masked_pair_ws(const void* A, int lda, const void* W, int ldw, void* C, int ldc, int M, int N, int K,
                                            const void* A2, int lda2, const void* W2, int ldw2, float drop_p, uint32_t seed,
                                            void* ws, int64_t ws_bytes, void* stream) {
  return masked_pair_impl(A, lda, W, ldw, C, ldc, M, N, K, A2, lda2, W2, ldw2, drop_p, seed, ws, ws_bytes, stream, VLB_ACT_NONE, nullptr, 0);
}

extern "C" int vlb_gemm_masked_pair_swiglu_bwd(const void* dY, int lddy, const void* Wt, int ldw, const void* gu, int ldgu, void* dgu,
                                               int lddgu, int M, int ff, int K, const void* U, int ldu, const void* At, int ldat,
                                               float drop_p, uint32_t seed, void* ws, int64_t ws_bytes, void* stream) {
  VLB_REQUIRE(gu && dgu, "gemm_masked_pair_swiglu_bwd: null activation pointers");
  VLB_REQUIRE(ldgu >= 2 * ff && lddgu >= 2 * ff && ldgu % 8 == 0 && lddgu % 8 == 0 && ff % 8 == 0 && ((uintptr_t)gu % 16) == 0 && ((uintptr_t)dgu % 16) == 0,
              "gemm_masked_pair_swiglu_bwd: [gate|up] rows must hold 2*ff columns; gu and d gu rows 16-byte aligned (ff=%d ldgu=%d lddgu=%d)", ff, ldgu, lddgu);
  return masked_pair_impl(dY, lddy, Wt, ldw, dgu, lddgu, M, ff, K, U, ldu, At, ldat, drop_p, seed, ws, ws_bytes, stream,
                          VLB_ACT_SWIGLU_BWD, gu, ldgu);
}

#ifdef VLB_TOOLS
// tuning hooks, libvlb_tools.so only: kernel variant / forced tile
extern "C" void vlb_gemm_set_variant(int variant, int force_tile) {
  g_variant = variant & 0xff;     // 3 = default (auto)
  g_force_tile = force_tile;
  g_tail_split = (variant & 0x100) ? 0 : 1;    // bit 8 disables the tail split (A/B)
  g_tail_splitk = (variant & 0x200) ? 0 : 1;   // bit 9 disables the split-K tail (A/B)
  g_order_auto = (variant & 0x2000) ? 0 : 1;
  g_tile_order = ((variant >> 10) & 7) ^ 3;       // variant word 3 = product default (order 3)
}
#endif

extern "C" int vlb_transpose_bf16(const void* in, void* out, int R, int C, void* stream) {
  VLB_REQUIRE(in && out && R > 0 && C > 0, "transpose: bad args");
  dim3 grid((C + 31) / 32, (R + 31) / 32), block(32, 8);
  hipLaunchKernelGGL(transpose_kernel, grid, block, 0, as_stream(stream), (const bf16*)in, (bf16*)out, R, C);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}
