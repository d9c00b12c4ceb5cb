// Closed-form fit of the ridge head (RidgeRegressionLayer, src/utils.py:59-73) from the frozen-feature cache, DESIGN §5.3.5.
//
//   J(W, b) = 1/(N V) sum_n || W z_n + b - y_n ||^2 + l2_lambda ||W||_F^2         (z bf16 [E], y fp32 [V])
//   (Zc^T Zc + l2_lambda N V I) W^T = Zc^T Yc,   b = ybar - W zbar
//
// Everything here is fp64: the sums G = Z^T Z [E,E], C = Y^T Z [V,E], sz = colsum(Z), sy = colsum(Y) (products of a bf16
// and a bf16 / fp32 value are exact in fp64), the centring, the lower Cholesky factor and the two triangular solves.
// Plain fp64 FMAs (v_fma_f64), no MFMA: fp64 time is not what these epochs wait for (§5.3.5 has the figures).
// No atomics anywhere: every output element is owned by one thread and summed in one fixed order, so two runs give the same
// bits.  All stores are vector stores.
#include "common.hpp"

typedef double f64x2 __attribute__((ext_vector_type(2)));

namespace {

constexpr int TS = 64;        // output tile edge of the tile kernels (256 threads, 4 x 4 results each)
constexpr int GK = 32;        // rows of z / y staged per step of the Gram kernel
constexpr int FK = 16;        // k-slice of the fp64 tile kernel
constexpr int NB = 64;        // Cholesky / substitution block
constexpr int LP = NB + 1;    // LDS row pitch (doubles) of a 64 x 64 block: column walks hit 64 different banks

// ---------------------------------------------------------------- Gram pass: D[M,N] += A^T B over n rows
// A is [n, M] (bf16 for G: the same z; fp32 for C: y, pitch lda), B = z bf16 [n, N], D fp64 [M, N] row-major, pitch ldd.
// grid (ceil(N/64), ceil(M/64)), 256 threads.  A 32-row slab of each operand is staged in LDS in its own narrow type (one
// 16-byte global load and one 16-byte LDS store per lane where the pitch allows, contiguous over the lanes: no bank
// conflict) and widened when read: per k a thread reads its 4 A and 4 B values as one 8- or 16-byte LDS read (16 lanes
// contiguous, the 4 lane rows broadcast).  The rows are summed in ascending order into 16 fp64 accumulators per thread.
__device__ __forceinline__ double widen(bf16 x) { return (double)(float)x; }
__device__ __forceinline__ double widen(float x) { return (double)x; }

// MASK (the target-weighted fit; T = float): column c0 + j of src is read through a select on keep[c0 + j] > 0,
// else +0.0f - never a product, so a NaN / Inf in a masked column stays out of the slab.  A thread's columns are the same in
// every step of the chunk loop (256 % (TS / PER) == 0), so its PER flags are read once; keep is not read at c0 + j >= ncols.
template <typename T, bool MASK = false>
__device__ __forceinline__ void stage_slab(const T* __restrict__ src, int64_t ld, int r0, int n, int c0, int ncols, T* lds,
                                           const float* __restrict__ keep = nullptr) {
  constexpr int PER = 16 / (int)sizeof(T);                 // elements of one 16-byte access
  constexpr int CHUNKS = GK * TS / PER;                    // 256 (bf16) or 512 (fp32)
  static_assert(256 % (TS / PER) == 0, "a thread keeps its columns over the chunk loop");
  const bool vec = ld % PER == 0 && ((uintptr_t)src & 15) == 0 && c0 + TS <= ncols;      // block-uniform
  [[maybe_unused]] bool kp[PER];
  if constexpr (MASK) {
    static_assert(sizeof(T) == 4, "the masked slab is the fp32 target slab");
    const int kc = c0 + ((int)threadIdx.x % (TS / PER)) * PER;
#pragma unroll
    for (int i = 0; i < PER; ++i) kp[i] = kc + i < ncols && keep[kc + i] > 0.f;
  }
#pragma unroll
  for (int c = threadIdx.x; c < CHUNKS; c += 256) {
    const int r = c / (TS / PER), col = (c % (TS / PER)) * PER;
    T* dst = lds + r * TS + col;
    if (vec) {
      u32x4 v = {0u, 0u, 0u, 0u};
      if (r0 + r < n) v = *reinterpret_cast<const u32x4*>(src + (int64_t)(r0 + r) * ld + c0 + col);
      if constexpr (MASK) {
#pragma unroll
        for (int i = 0; i < PER; ++i) v[i] = kp[i] ? v[i] : 0u;
      }
      *reinterpret_cast<u32x4*>(dst) = v;
    } else {
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        bool in = r0 + r < n && c0 + col + i < ncols;
        if constexpr (MASK) in = in && kp[i];
        dst[i] = in ? src[(int64_t)(r0 + r) * ld + c0 + col + i] : (T)0.f;
      }
    }
  }
}

template <typename TA, bool MASK>
__device__ __forceinline__ void gram_tile_body(const TA* __restrict__ A, int64_t lda, const bf16* __restrict__ Bz, int64_t ldb,
                                               double* __restrict__ D, int64_t ldd, int n, int M, int N,
                                               const float* __restrict__ keep) {
  __shared__ __attribute__((aligned(16))) TA As[GK * TS];
  __shared__ __attribute__((aligned(16))) bf16 Bs[GK * TS];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int i0 = blockIdx.y * TS, j0 = blockIdx.x * TS;
  double acc[4][4] = {};
  for (int r0 = 0; r0 < n; r0 += GK) {
    __syncthreads();
    stage_slab<TA, MASK>(A, lda, r0, n, i0, M, As, keep);
    stage_slab<bf16>(Bz, ldb, r0, n, j0, N, Bs);
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < GK; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = widen(As[k * TS + ty * 4 + i]);
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = widen(Bs[k * TS + tx * 4 + j]);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
  }
  const int col = j0 + tx * 4;
  const bool vec = ldd % 2 == 0 && ((uintptr_t)D & 15) == 0 && col + 4 <= N;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i0 + ty * 4 + i;
    if (row >= M) continue;
    double* d = D + (int64_t)row * ldd + col;
    if (vec) {
      f64x2* d2 = reinterpret_cast<f64x2*>(d);
      f64x2 lo = d2[0], hi = d2[1];
      lo.x += acc[i][0]; lo.y += acc[i][1]; hi.x += acc[i][2]; hi.y += acc[i][3];
      d2[0] = lo; d2[1] = hi;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col + j < N) d[j] += acc[i][j];
    }
  }
}

template <typename TA>
__global__ __launch_bounds__(256) void gram_tile_kernel(const TA* __restrict__ A, int64_t lda, const bf16* __restrict__ Bz,
                                                        int64_t ldb, double* __restrict__ D, int64_t ldd, int n, int M, int N) {
  gram_tile_body<TA, false>(A, lda, Bz, ldb, D, ldd, n, M, N, nullptr);
}
// C [V,E] += y^T z with the rows of C (the columns of y) read through keep: a masked row of C gets +0.0 added
__global__ __launch_bounds__(256) void gram_tile_masked_kernel(const float* __restrict__ A, int64_t lda, const bf16* __restrict__ Bz,
                                                               int64_t ldb, double* __restrict__ D, int64_t ldd, int n, int M, int N,
                                                               const float* __restrict__ keep) {
  gram_tile_body<float, true>(A, lda, Bz, ldb, D, ldd, n, M, N, keep);
}

// s[c] += sum over the n rows (ascending) of x[r, c]: one thread per column, lanes on consecutive columns.
// MASK: x[r, c] through the select on keep[c] > 0 (else +0.0f, the element is not loaded); SQ: the squares (an fp32 square is
// exact in fp64), colsumsq_f64_kernel's loop
template <typename T, bool MASK, bool SQ>
__device__ __forceinline__ void colsum_f64_body(const T* __restrict__ x, int64_t ld, double* __restrict__ s, int n, int ncols,
                                                const float* __restrict__ keep) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncols) return;
  [[maybe_unused]] bool kp = true;
  if constexpr (MASK) kp = keep[c] > 0.f;
  double t = 0.0;
  for (int r = 0; r < n; ++r) {
    T xv;
    if constexpr (MASK) xv = kp ? x[(int64_t)r * ld + c] : (T)0.f;
    else xv = x[(int64_t)r * ld + c];
    const double w = widen(xv);
    if constexpr (SQ) t = fma(w, w, t);
    else t += w;
  }
  s[c] += t;
}
template <typename T>
__global__ __launch_bounds__(256) void colsum_f64_kernel(const T* __restrict__ x, int64_t ld, double* __restrict__ s, int n,
                                                         int ncols) {
  colsum_f64_body<T, false, false>(x, ld, s, n, ncols, nullptr);
}
template <bool SQ>
__global__ __launch_bounds__(256) void colsum_masked_f64_kernel(const float* __restrict__ x, int64_t ld, double* __restrict__ s,
                                                                int n, int ncols, const float* __restrict__ keep) {
  colsum_f64_body<float, true, SQ>(x, ld, s, n, ncols, keep);
}

// ---------------------------------------------------------------- fp64 tile kernel: D[M,N] -= P Q^T  (or P Q, QT)
//   D[i,j] -= sum_{k<K} P[i*ldp + k] * (QT ? Q[k*ldq + j] : Q[j*ldq + k])
// The Cholesky trailing update (P = Q = the panel below the diagonal block, lower = 1: only tiles that touch the lower
// triangle run and only elements with j <= i are stored, D's (0,0) being a diagonal element) and the block updates of the
// forward (P = solved block of X, Q = rows of L) and back (QT: Q = columns of L) substitution.
// grid (ceil(N/64), ceil(M/64)), 256 threads.  Both operands are staged k-major in LDS with a 65-double pitch: the fill's
// 8-byte stores (4 rows x 4 k-quads per 16 lanes; QT: 16 consecutive columns) and the reads (16 consecutive doubles per
// lane row, the other lane rows broadcast) touch every bank at most once per lane group.  A thread owns rows ty + 16 i and
// columns tx + 16 j, so its global accesses to D are 128 contiguous bytes per 16 lanes.
// A non-zero *info (a failed factorisation) turns the kernel into a no-op.
template <bool QT>
__global__ __launch_bounds__(256) void tile_sub_f64_kernel(double* __restrict__ D, int64_t ldd, const double* P, int64_t ldp,
                                                           const double* Q, int64_t ldq, int M, int N, int K, int lower,
                                                           const int* __restrict__ info) {
  __shared__ double Ps[FK * LP];
  __shared__ double Qs[FK * LP];
  if (info && *info != 0) return;
  const int i0 = blockIdx.y * TS, j0 = blockIdx.x * TS;
  if (lower && j0 > i0 + TS - 1) return;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4] = {};
  const bool pvec = ldp % 2 == 0 && ((uintptr_t)P & 15) == 0, qvec = ldq % 2 == 0 && ((uintptr_t)Q & 15) == 0;
  for (int kc = 0; kc < K; kc += FK) {
    __syncthreads();
    {   // rows of P (and of Q): lane t -> row t / 4, k-quad t % 4; two 16-byte loads where aligned
      const int r = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 4, k = kc + kq;
      double v[4] = {0.0, 0.0, 0.0, 0.0};
      if (i0 + r < M) {
        const double* p = P + (int64_t)(i0 + r) * ldp + k;
        if (pvec && k + 4 <= K) {
          const f64x2 lo = reinterpret_cast<const f64x2*>(p)[0], hi = reinterpret_cast<const f64x2*>(p)[1];
          v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) if (k + i < K) v[i] = p[i];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) Ps[(kq + i) * LP + r] = v[i];
      if (!QT) {
        double w[4] = {0.0, 0.0, 0.0, 0.0};
        if (j0 + r < N) {
          const double* q = Q + (int64_t)(j0 + r) * ldq + k;
          if (qvec && k + 4 <= K) {
            const f64x2 lo = reinterpret_cast<const f64x2*>(q)[0], hi = reinterpret_cast<const f64x2*>(q)[1];
            w[0] = lo.x; w[1] = lo.y; w[2] = hi.x; w[3] = hi.y;
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) if (k + i < K) w[i] = q[i];
          }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) Qs[(kq + i) * LP + r] = w[i];
      } else {   // Q is k-major already: lane t -> k t / 16, columns t % 16 + 16 i (128 contiguous bytes per 16 lanes)
        const int kk = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int j = tx + 16 * i;
          Qs[kk * LP + j] = (kc + kk < K && j0 + j < N) ? Q[(int64_t)(kc + kk) * ldq + j0 + j] : 0.0;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FK; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = Ps[k * LP + ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Qs[k * LP + tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i0 + ty + 16 * i;
    if (row >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = j0 + tx + 16 * j;
      if (col < N && (!lower || col <= row)) D[(int64_t)row * ldd + col] -= acc[i][j];
    }
  }
}

// ---------------------------------------------------------------- Cholesky: the nb x nb diagonal block, in LDS
// One block of 256 threads, right-looking.  Only the lower triangle is read and written.  A pivot that is not > 0 (a NaN
// fails the comparison too) puts its 1-based index into *info (first failure wins) and ends the kernel before anything of
// this block is written back; every later kernel of the factorisation and of a solve returns at once on *info != 0.
__global__ __launch_bounds__(256) void chol_block_kernel(double* __restrict__ A, int64_t lda, int k0, int nb, int* __restrict__ info) {
  __shared__ double Ls[NB * LP];
  if (*info != 0) return;
  double* blk = A + (int64_t)k0 * lda + k0;
  for (int e = threadIdx.x; e < nb * nb; e += 256) {
    const int i = e / nb, j = e % nb;
    if (j <= i) Ls[i * LP + j] = blk[(int64_t)i * lda + j];
  }
  __syncthreads();
  for (int j = 0; j < nb; ++j) {
    const double d = Ls[j * LP + j];
    if (!(d > 0.0)) {                       // uniform: every thread reads the same value
      if (threadIdx.x == 0) *info = k0 + j + 1;
      return;
    }
    const double s = sqrt(d);
    __syncthreads();
    if (threadIdx.x == 0) Ls[j * LP + j] = s;
    for (int i = j + 1 + threadIdx.x; i < nb; i += 256) Ls[i * LP + j] /= s;
    __syncthreads();
    const int m = nb - j - 1;               // trailing square (rows, columns j+1 .. nb-1), lower part
    for (int e = threadIdx.x; e < m * m; e += 256) {
      const int i = j + 1 + e / m, c = j + 1 + e % m;
      if (c <= i) Ls[i * LP + c] = fma(-Ls[i * LP + j], Ls[c * LP + j], Ls[i * LP + c]);
    }
    __syncthreads();
  }
  for (int e = threadIdx.x; e < nb * nb; e += 256) {
    const int i = e / nb, j = e % nb;
    if (j <= i) blk[(int64_t)i * lda + j] = Ls[i * LP + j];
  }
}

// ---------------------------------------------------------------- substitution with one diagonal block, a row per thread
// X[r, k0 .. k0+nb) <- that row solved against L11 = L[k0.., k0..) (nb x nb, lower):
//   !BACK: x L11^T = a, i.e. x_j = (a_j - sum_{k<j} x_k L11[j,k]) / L11[j,j]    (Cholesky panel below the block; forward solve)
//    BACK: x L11   = a, i.e. x_j = (a_j - sum_{k>j} x_k L11[k,j]) / L11[j,j]    (back solve)
// L11 sits in LDS (T[j][k] = the coefficient of x_k in equation j; every lane reads the same word: a broadcast), padded to
// 64 x 64 with the identity so the loops have constant bounds and the row lives in registers.  grid ceil(rows/256).
template <bool BACK>
__global__ __launch_bounds__(256) void tri_rows_kernel(double* __restrict__ X, int64_t ldx, int nrows, const double* L, int64_t ldl,
                                                       int k0, int nb, const int* __restrict__ info) {
  __shared__ double T[NB * LP];
  if (*info != 0) return;
  const double* blk = L + (int64_t)k0 * ldl + k0;
  for (int e = threadIdx.x; e < NB * NB; e += 256) {
    const int j = e / NB, k = e % NB;          // consecutive lanes: consecutive k
    double v = j == k ? 1.0 : 0.0;
    if (j < nb && k < nb) {
      if (!BACK && k <= j) v = blk[(int64_t)j * ldl + k];
      if (BACK && k >= j) v = blk[(int64_t)k * ldl + j];
    }
    T[j * LP + k] = v;
  }
  __syncthreads();
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= nrows) return;
  double* row = X + (int64_t)r * ldx + k0;
  double x[NB];
  const bool vec = nb == NB && ldx % 2 == 0 && ((uintptr_t)(X + k0) & 15) == 0;
  if (vec) {
#pragma unroll
    for (int k = 0; k < NB; k += 2) {
      const f64x2 v = *reinterpret_cast<const f64x2*>(row + k);
      x[k] = v.x; x[k + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NB; ++k) x[k] = k < nb ? row[k] : 0.0;
  }
  if (!BACK) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      double t = x[j];
#pragma unroll
      for (int k = 0; k < j; ++k) t = fma(-x[k], T[j * LP + k], t);
      x[j] = t / T[j * LP + j];
    }
  } else {
#pragma unroll
    for (int j = NB - 1; j >= 0; --j) {
      double t = x[j];
#pragma unroll
      for (int k = NB - 1; k > j; --k) t = fma(-x[k], T[j * LP + k], t);
      x[j] = t / T[j * LP + j];
    }
  }
  if (vec) {
#pragma unroll
    for (int k = 0; k < NB; k += 2) {
      f64x2 v = {x[k], x[k + 1]};
      *reinterpret_cast<f64x2*>(row + k) = v;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NB; ++k) if (k < nb) row[k] = x[k];
  }
}

// ---------------------------------------------------------------- the ridge system and what is read off its solution
// A[i,j] = G[i,j] - sz[i] sz[j] / N + (i == j) ridge   (ridge = l2_lambda N V, formed on the host in fp64), full square
__global__ __launch_bounds__(256) void ridge_form_a_kernel(const double* __restrict__ G, const double* __restrict__ sz,
                                                           double* __restrict__ A, int E, double inv_n, double ridge) {
  const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
  if (j >= E) return;
  double v = G[(int64_t)i * E + j] - sz[i] * sz[j] * inv_n;
  if (i == j) v += ridge;
  A[(int64_t)i * E + j] = v;
}
// R[v,e] = C[v,e] - sy[v] sz[e] / N
__global__ __launch_bounds__(256) void ridge_form_r_kernel(const double* __restrict__ C, const double* __restrict__ sz,
                                                           const double* __restrict__ sy, double* __restrict__ R, int E,
                                                           double inv_n) {
  const int e = blockIdx.x * 256 + threadIdx.x, v = blockIdx.y;
  if (e >= E) return;
  R[(int64_t)v * E + e] = C[(int64_t)v * E + e] - sy[v] * sz[e] * inv_n;
}
// The factorisation sees only the features.  A NaN / Inf target reaches C and sy alone (sy[v] is not finite exactly when
// column v of y holds one), so it is looked for here: the first such column v is reported as *info = -(v + 1), unless the
// factorisation has failed already.  One thread, ascending v: the answer does not depend on scheduling.
__global__ void ridge_check_targets_kernel(const double* __restrict__ sy, int V, int* __restrict__ info) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || *info != 0) return;
  for (int v = 0; v < V; ++v)
    if (!isfinite(sy[v])) {
      *info = -(v + 1);
      return;
    }
}
// W[v,:] = fp32(X[v,:]),  b[v] = fp32(sy[v] / N - (X[v,:] . sz) / N): one block per v; the dot product is summed per thread
// over e = t, t + 256, ... and then over the 256 threads in ascending order (fixed, no atomics).  No-op on *info != 0.
// With ``choice`` (vlb_ridge_solve_rows) only the rows with choice[v] == want are written, by the same
// arithmetic; the other rows' blocks return at once and their bytes in W and b stay as they are.
__global__ __launch_bounds__(256) void ridge_finish_kernel(const double* __restrict__ X, const double* __restrict__ sz,
                                                           const double* __restrict__ sy, float* __restrict__ W,
                                                           float* __restrict__ b, int E, double inv_n,
                                                           const int* __restrict__ info, const int* __restrict__ choice,
                                                           int want) {
  __shared__ double part[256];
  if (*info != 0) return;
  const int v = blockIdx.x;
  if (choice && choice[v] != want) return;              // block-uniform
  double t = 0.0;
  for (int e = threadIdx.x; e < E; e += 256) {
    const double x = X[(int64_t)v * E + e];
    W[(int64_t)v * E + e] = (float)x;
    t = fma(x, sz[e], t);
  }
  part[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int i = 0; i < 256; ++i) s += part[i];
    b[v] = (float)(sy[v] * inv_n - s * inv_n);
  }
}

// ---------------------------------------------------------------- blocked K-fold CV of l2_lambda
// s[c] += sum over the n rows (ascending) of y[r, c]^2: colsum_f64_kernel's twin (an fp32 square is exact in fp64)
__global__ __launch_bounds__(256) void colsumsq_f64_kernel(const float* __restrict__ y, int64_t ld, double* __restrict__ s, int n,
                                                           int ncols) {
  colsum_f64_body<float, false, true>(y, ld, s, n, ncols, nullptr);
}
// out[i] = sum over j != skip (ascending) of parts[j * stride + i]: one thread per element, lanes on consecutive elements
__global__ __launch_bounds__(256) void sum_except_f64_kernel(const double* __restrict__ parts, int64_t stride, int count, int skip,
                                                             double* __restrict__ out, int64_t numel) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= numel) return;
  double t = 0.0;
  for (int j = 0; j < count; ++j)
    if (j != skip) t += parts[(int64_t)j * stride + i];
  out[i] = t;
}
// vy[v] = syy[v] - sy[v]^2 / n
__global__ __launch_bounds__(256) void cv_vy_kernel(const double* __restrict__ syy, const double* __restrict__ sy,
                                                    double* __restrict__ vy, int V, double inv_n) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v < V) vy[v] = syy[v] - sy[v] * sy[v] * inv_n;
}
// The quadratic form vp[v] = X[v,:] Gc X[v,:]^T, one partial per (target, 64-column tile):
//   ws[v * nct + c] = sum_{j in tile c} (sum_k X[v,k] Gc[k,j]) X[v,j],   nct = ceil(E / 64)
// tile_sub_f64_kernel<QT>'s loop (P = X rows, Q = Gc k-major; the same staging, the same 65-double pitch, the same 16-lane
// reads), but the 64 x 64 tile of T = X Gc stays in the accumulators: each is multiplied by X[v,j], a thread adds its four
// columns tx, tx + 16, tx + 32, tx + 48 in that order, and one thread per target adds the 16 lanes' sums in ascending tx
// (LDS, pitch 17: 32 lanes on 32 different bank pairs).  grid (nct, ceil(V/64)), 256 threads.  No-op on *info != 0.
__global__ __launch_bounds__(256) void cv_quad_tile_kernel(const double* __restrict__ X, const double* __restrict__ Gc,
                                                           double* __restrict__ ws, int E, int V, const int* __restrict__ info) {
  __shared__ double Ps[FK * LP];
  __shared__ double Qs[FK * LP];
  __shared__ double red[TS * 17];
  if (*info != 0) return;
  const int i0 = blockIdx.y * TS, j0 = blockIdx.x * TS;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  double acc[4][4] = {};
  const bool pvec = E % 2 == 0 && ((uintptr_t)X & 15) == 0;
  for (int kc = 0; kc < E; kc += FK) {
    __syncthreads();
    {   // rows of X: lane t -> row t / 4, k-quad t % 4
      const int r = threadIdx.x >> 2, kq = (threadIdx.x & 3) * 4, k = kc + kq;
      double v[4] = {0.0, 0.0, 0.0, 0.0};
      if (i0 + r < V) {
        const double* p = X + (int64_t)(i0 + r) * E + k;
        if (pvec && k + 4 <= E) {
          const f64x2 lo = reinterpret_cast<const f64x2*>(p)[0], hi = reinterpret_cast<const f64x2*>(p)[1];
          v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i) if (k + i < E) v[i] = p[i];
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) Ps[(kq + i) * LP + r] = v[i];
      // Gc is k-major already: lane t -> k t / 16, columns t % 16 + 16 i (128 contiguous bytes per 16 lanes)
      const int kk = threadIdx.x >> 4;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = tx + 16 * i;
        Qs[kk * LP + j] = (kc + kk < E && j0 + j < E) ? Gc[(int64_t)(kc + kk) * E + j0 + j] : 0.0;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FK; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = Ps[k * LP + ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = Qs[k * LP + tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = i0 + ty + 16 * i;
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = j0 + tx + 16 * j;
      const double x = (row < V && col < E) ? X[(int64_t)row * E + col] : 0.0;
      t = fma(acc[i][j], x, t);
    }
    red[(ty + 16 * i) * 17 + tx] = t;
  }
  __syncthreads();
  if (threadIdx.x < TS && i0 + threadIdx.x < V) {
    double s = 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) s += red[threadIdx.x * 17 + t];
    ws[(int64_t)(i0 + threadIdx.x) * gridDim.x + blockIdx.x] = s;
  }
}
// r[v] = cov / sqrt(vp vy) clipped to [-1, 1], 0 unless vp > 0 and vy > 0:  vp = the nct partials of ws in ascending order,
// cov = X[v,:] . Rc[v,:] summed as ridge_finish_kernel sums (per thread over e = t, t + 256, ..., then the 256 threads in
// ascending order).  One block per v.  No-op on *info != 0.
// ROWS (vlb_ridge_cv_score_rows): only the blocks with choice[v] == want run, by the same arithmetic; every
// other r_out[v] keeps its bytes - ridge_finish_kernel's pattern.
template <bool ROWS>
__device__ __forceinline__ void cv_finish_body(const double* __restrict__ X, const double* __restrict__ Rc,
                                               const double* __restrict__ vy, const double* __restrict__ ws,
                                               double* __restrict__ r_out, int E, int nct, const int* __restrict__ info,
                                               const int* __restrict__ choice, int want) {
  __shared__ double part[256];
  if (*info != 0) return;
  const int v = blockIdx.x;
  if constexpr (ROWS) {
    if (choice[v] != want) return;                      // block-uniform
  }
  double t = 0.0;
  for (int e = threadIdx.x; e < E; e += 256) t = fma(X[(int64_t)v * E + e], Rc[(int64_t)v * E + e], t);
  part[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double cov = 0.0, vp = 0.0;
    for (int i = 0; i < 256; ++i) cov += part[i];
    for (int c = 0; c < nct; ++c) vp += ws[(int64_t)v * nct + c];
    const double y2 = vy[v];
    double r = 0.0;
    if (vp > 0.0 && y2 > 0.0) {
      r = cov / sqrt(vp * y2);
      r = r > 1.0 ? 1.0 : r < -1.0 ? -1.0 : r;
    }
    r_out[v] = r;
  }
}
__global__ __launch_bounds__(256) void cv_finish_kernel(const double* __restrict__ X, const double* __restrict__ Rc,
                                                        const double* __restrict__ vy, const double* __restrict__ ws,
                                                        double* __restrict__ r_out, int E, int nct,
                                                        const int* __restrict__ info) {
  cv_finish_body<false>(X, Rc, vy, ws, r_out, E, nct, info, nullptr, 0);
}
__global__ __launch_bounds__(256) void cv_finish_rows_kernel(const double* __restrict__ X, const double* __restrict__ Rc,
                                                             const double* __restrict__ vy, const double* __restrict__ ws,
                                                             double* __restrict__ r_out, int E, int nct,
                                                             const int* __restrict__ info, const int* __restrict__ choice,
                                                             int want) {
  cv_finish_body<true>(X, Rc, vy, ws, r_out, E, nct, info, choice, want);
}

// ---------------------------------------------------------------- l2_lambda per target
// One head's slice of the held-out table, [K,L,V]: rmean[i,v] = (sum_k table[k,i,v], ascending k, from 0) / K for every grid
// point; choice[v] = the grid point with the largest rmean among those with ok[i] != 0 (an excluded point is never compared,
// whatever it holds), an exact tie going to the larger grid[i]; rbest[v] = its rmean.  No point allowed: choice -1, rbest NaN.
// One thread per target, lanes on consecutive targets: every load and store is contiguous over the lanes.
__global__ __launch_bounds__(256) void cv_select_kernel(const double* __restrict__ table, const double* __restrict__ grid,
                                                        const int* __restrict__ ok, double* __restrict__ rmean,
                                                        int* __restrict__ choice, double* __restrict__ rbest, int K, int L, int V) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= V) return;
  const double k_d = (double)K;
  int best = -1;
  double rb = __builtin_nan(""), gb = 0.0;
  for (int i = 0; i < L; ++i) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) s += table[((int64_t)k * L + i) * V + v];
    const double m = s / k_d;
    rmean[(int64_t)i * V + v] = m;
    if (ok[i] == 0) continue;
    const double g = grid[i];
    if (best < 0 || m > rb || (m == rb && g > gb)) { best = i; rb = m; gb = g; }
  }
  choice[v] = best;
  rbest[v] = rb;
}

inline dim3 tiles(int M, int N) { return dim3((N + TS - 1) / TS, (M + TS - 1) / TS); }

}  // namespace

// ---------------------------------------------------------------- C-ABI
extern "C" int vlb_ridge_gram_accumulate(const void* z, const float* y, int ldy, double* G, double* C, double* sz, double* sy,
                                         int n, int E, int V, void* stream) {
  VLB_REQUIRE(z && y && G && C && sz && sy, "ridge_gram_accumulate: null argument");
  VLB_REQUIRE(n >= 1 && E >= 1 && V >= 1 && ldy >= V, "ridge_gram_accumulate: bad shape n=%d E=%d V=%d ldy=%d", n, E, V, ldy);
  hipStream_t st = as_stream(stream);
  const bf16* zz = (const bf16*)z;
  hipLaunchKernelGGL(gram_tile_kernel<bf16>, tiles(E, E), dim3(256), 0, st, zz, (int64_t)E, zz, (int64_t)E, G, (int64_t)E, n, E, E);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(gram_tile_kernel<float>, tiles(V, E), dim3(256), 0, st, y, (int64_t)ldy, zz, (int64_t)E, C, (int64_t)E, n, V, E);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum_f64_kernel<bf16>, dim3((E + 255) / 256), dim3(256), 0, st, zz, (int64_t)E, sz, n, E);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum_f64_kernel<float>, dim3((V + 255) / 256), dim3(256), 0, st, y, (int64_t)ldy, sy, n, V);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// the target-weighted fit: vlb_ridge_gram_accumulate's four launches, y read through keep
extern "C" int vlb_ridge_gram_accumulate_masked(const void* z, const float* y, int ldy, const float* keep, double* G, double* C,
                                                double* sz, double* sy, int n, int E, int V, void* stream) {
  VLB_REQUIRE(z && y && keep && G && C && sz && sy, "ridge_gram_accumulate_masked: null argument");
  VLB_REQUIRE(n >= 1 && E >= 1 && V >= 1 && ldy >= V, "ridge_gram_accumulate_masked: bad shape n=%d E=%d V=%d ldy=%d", n, E, V, ldy);
  VLB_REQUIRE(((uintptr_t)keep & 3) == 0, "ridge_gram_accumulate_masked: keep is not 4-byte aligned");
  hipStream_t st = as_stream(stream);
  const bf16* zz = (const bf16*)z;
  hipLaunchKernelGGL(gram_tile_kernel<bf16>, tiles(E, E), dim3(256), 0, st, zz, (int64_t)E, zz, (int64_t)E, G, (int64_t)E, n, E, E);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(gram_tile_masked_kernel, tiles(V, E), dim3(256), 0, st, y, (int64_t)ldy, zz, (int64_t)E, C, (int64_t)E, n, V, E,
                     keep);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum_f64_kernel<bf16>, dim3((E + 255) / 256), dim3(256), 0, st, zz, (int64_t)E, sz, n, E);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(colsum_masked_f64_kernel<false>, dim3((V + 255) / 256), dim3(256), 0, st, y, (int64_t)ldy, sy, n, V, keep);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

static int chol_launch(double* A, int n, int64_t lda, int* info, hipStream_t st) {
  for (int k0 = 0; k0 < n; k0 += NB) {
    const int nb = n - k0 < NB ? n - k0 : NB, m = n - k0 - nb;          // m > 0 only below a full block
    hipLaunchKernelGGL(chol_block_kernel, dim3(1), dim3(256), 0, st, A, lda, k0, nb, info);
    VLB_LAUNCH_CHECK();
    if (m <= 0) break;
    double* below = A + (int64_t)(k0 + nb) * lda + k0;                   // A21 -> L21 = A21 L11^-T
    hipLaunchKernelGGL(tri_rows_kernel<false>, dim3((m + 255) / 256), dim3(256), 0, st, A + (int64_t)(k0 + nb) * lda, lda, m, A, lda,
                       k0, nb, info);
    VLB_LAUNCH_CHECK();
    double* trail = A + (int64_t)(k0 + nb) * lda + (k0 + nb);            // A22 -= L21 L21^T (lower)
    hipLaunchKernelGGL(tile_sub_f64_kernel<false>, tiles(m, m), dim3(256), 0, st, trail, lda, below, lda, below, lda, m, m, nb, 1, info);
    VLB_LAUNCH_CHECK();
  }
  return VLB_OK;
}

extern "C" int vlb_chol_f64(double* A, int n, int lda, int* info, void* stream) {
  VLB_REQUIRE(A && info, "chol_f64: null argument");
  VLB_REQUIRE(n >= 1 && lda >= n, "chol_f64: bad shape n=%d lda=%d", n, lda);
  hipStream_t st = as_stream(stream);
  if (hipMemsetAsync(info, 0, sizeof(int), st) != hipSuccess) {
    vlb_set_error("chol_f64: clearing info failed");
    return VLB_ERR_LAUNCH;
  }
  return chol_launch(A, n, lda, info, st);
}

extern "C" int vlb_chol_solve_f64(const double* L, int ldl, double* X, int n, int nrhs, int ldx, const int* info, void* stream) {
  VLB_REQUIRE(L && X && info, "chol_solve_f64: null argument");
  VLB_REQUIRE(n >= 1 && nrhs >= 1 && ldl >= n && ldx >= n, "chol_solve_f64: bad shape n=%d nrhs=%d ldl=%d ldx=%d", n, nrhs, ldl, ldx);
  hipStream_t st = as_stream(stream);
  const dim3 rows((nrhs + 255) / 256);
  for (int k0 = 0; k0 < n; k0 += NB) {          // L y = r, block column by block column
    const int nb = n - k0 < NB ? n - k0 : NB, m = n - k0 - nb;
    hipLaunchKernelGGL(tri_rows_kernel<false>, rows, dim3(256), 0, st, X, (int64_t)ldx, nrhs, L, (int64_t)ldl, k0, nb, info);
    VLB_LAUNCH_CHECK();
    if (m > 0) {                                 // X[:, rest] -= X[:, blk] L[rest, blk]^T
      hipLaunchKernelGGL(tile_sub_f64_kernel<false>, tiles(nrhs, m), dim3(256), 0, st, X + k0 + nb, (int64_t)ldx, X + k0,
                         (int64_t)ldx, L + (int64_t)(k0 + nb) * ldl + k0, (int64_t)ldl, nrhs, m, nb, 0, info);
      VLB_LAUNCH_CHECK();
    }
  }
  for (int k0 = (n - 1) / NB * NB; k0 >= 0; k0 -= NB) {   // L^T x = y, from the last block up
    const int nb = n - k0 < NB ? n - k0 : NB;
    hipLaunchKernelGGL(tri_rows_kernel<true>, rows, dim3(256), 0, st, X, (int64_t)ldx, nrhs, L, (int64_t)ldl, k0, nb, info);
    VLB_LAUNCH_CHECK();
    if (k0 > 0) {                                // X[:, 0..k0) -= X[:, blk] L[blk, 0..k0)
      hipLaunchKernelGGL(tile_sub_f64_kernel<true>, tiles(nrhs, k0), dim3(256), 0, st, X, (int64_t)ldx, X + k0, (int64_t)ldx,
                         L + (int64_t)k0 * ldl, (int64_t)ldl, nrhs, k0, nb, 0, info);
      VLB_LAUNCH_CHECK();
    }
  }
  return VLB_OK;
}

// form, factor, solve, finish: vlb_ridge_solve (choice = nullptr: every row is written) and vlb_ridge_solve_rows (rows with
// choice[v] == want) run this one sequence of launches
static int ridge_solve_launch(const double* G, const double* C, const double* sz, const double* sy, int64_t N, double l2_lambda,
                              double* A_ws, double* X_ws, float* W_out, float* b_out, int* info, int E, int V, const int* choice,
                              int want, void* stream) {
  const double inv_n = 1.0 / (double)N, ridge = l2_lambda * (double)N * (double)V;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ridge_form_a_kernel, dim3((E + 255) / 256, E), dim3(256), 0, st, G, sz, A_ws, E, inv_n, ridge);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(ridge_form_r_kernel, dim3((E + 255) / 256, V), dim3(256), 0, st, C, sz, sy, X_ws, E, inv_n);
  VLB_LAUNCH_CHECK();
  if (int rc = vlb_chol_f64(A_ws, E, E, info, stream)) return rc;
  hipLaunchKernelGGL(ridge_check_targets_kernel, dim3(1), dim3(64), 0, st, sy, V, info);
  VLB_LAUNCH_CHECK();
  if (int rc = vlb_chol_solve_f64(A_ws, E, X_ws, E, V, E, info, stream)) return rc;
  hipLaunchKernelGGL(ridge_finish_kernel, dim3(V), dim3(256), 0, st, X_ws, sz, sy, W_out, b_out, E, inv_n, info, choice, want);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_ridge_solve(const double* G, const double* C, const double* sz, const double* sy, int64_t N, double l2_lambda,
                               double* A_ws, double* X_ws, float* W_out, float* b_out, int* info, int E, int V, void* stream) {
  VLB_REQUIRE(G && C && sz && sy && A_ws && X_ws && W_out && b_out && info, "ridge_solve: null argument");
  VLB_REQUIRE(E >= 1 && V >= 1 && N >= 1, "ridge_solve: bad shape E=%d V=%d N=%lld", E, V, (long long)N);
  VLB_REQUIRE(l2_lambda >= 0.0, "ridge_solve: l2_lambda=%g is negative", l2_lambda);
  return ridge_solve_launch(G, C, sz, sy, N, l2_lambda, A_ws, X_ws, W_out, b_out, info, E, V, nullptr, 0, stream);
}

// ---------------------------------------------------------------- C-ABI: l2_lambda per target
extern "C" int vlb_ridge_solve_rows(const double* G, const double* C, const double* sz, const double* sy, int64_t N,
                                    double l2_lambda, double* A_ws, double* X_ws, float* W_out, float* b_out, int* info, int E,
                                    int V, const int* choice, int want, void* stream) {
  VLB_REQUIRE(G && C && sz && sy && A_ws && X_ws && W_out && b_out && info && choice, "ridge_solve_rows: null argument");
  VLB_REQUIRE(E >= 1 && V >= 1 && N >= 1, "ridge_solve_rows: bad shape E=%d V=%d N=%lld", E, V, (long long)N);
  VLB_REQUIRE(l2_lambda >= 0.0, "ridge_solve_rows: l2_lambda=%g is negative", l2_lambda);
  VLB_REQUIRE(want >= 0, "ridge_solve_rows: want=%d is negative", want);
  return ridge_solve_launch(G, C, sz, sy, N, l2_lambda, A_ws, X_ws, W_out, b_out, info, E, V, choice, want, stream);
}

extern "C" int vlb_ridge_cv_select(const double* table, const double* grid, const int* ok, double* rmean, int* choice,
                                   double* rbest, int K, int L, int V, void* stream) {
  VLB_REQUIRE(table && grid && ok && rmean && choice && rbest, "ridge_cv_select: null argument");
  VLB_REQUIRE(K >= 1 && L >= 1 && V >= 1, "ridge_cv_select: bad shape K=%d L=%d V=%d", K, L, V);
  hipLaunchKernelGGL(cv_select_kernel, dim3((V + 255) / 256), dim3(256), 0, as_stream(stream), table, grid, ok, rmean, choice, rbest,
                     K, L, V);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// ---------------------------------------------------------------- C-ABI: blocked K-fold CV of l2_lambda
extern "C" int vlb_ridge_sumsq_accumulate(const float* y, int ldy, double* syy, int n, int V, void* stream) {
  VLB_REQUIRE(y && syy, "ridge_sumsq_accumulate: null argument");
  VLB_REQUIRE(n >= 1 && V >= 1 && ldy >= V, "ridge_sumsq_accumulate: bad shape n=%d V=%d ldy=%d", n, V, ldy);
  hipLaunchKernelGGL(colsumsq_f64_kernel, dim3((V + 255) / 256), dim3(256), 0, as_stream(stream), y, (int64_t)ldy, syy, n, V);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_ridge_sumsq_accumulate_masked(const float* y, int ldy, const float* keep, double* syy, int n, int V,
                                                 void* stream) {
  VLB_REQUIRE(y && keep && syy, "ridge_sumsq_accumulate_masked: null argument");
  VLB_REQUIRE(n >= 1 && V >= 1 && ldy >= V, "ridge_sumsq_accumulate_masked: bad shape n=%d V=%d ldy=%d", n, V, ldy);
  VLB_REQUIRE(((uintptr_t)keep & 3) == 0, "ridge_sumsq_accumulate_masked: keep is not 4-byte aligned");
  hipLaunchKernelGGL(colsum_masked_f64_kernel<true>, dim3((V + 255) / 256), dim3(256), 0, as_stream(stream), y, (int64_t)ldy, syy, n,
                     V, keep);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_f64_sum_except(const double* parts, int64_t stride, int count, int skip, double* out, int64_t numel,
                                  void* stream) {
  VLB_REQUIRE(parts && out, "f64_sum_except: null argument");
  VLB_REQUIRE(count >= 1 && skip >= -1 && skip < count && numel >= 1 && stride >= numel && numel <= ((int64_t)1 << 38),
              "f64_sum_except: bad shape count=%d skip=%d numel=%lld stride=%lld", count, skip, (long long)numel, (long long)stride);
  hipLaunchKernelGGL(sum_except_f64_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, as_stream(stream), parts, stride,
                     count, skip, out, numel);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int vlb_ridge_cv_center(const double* G_k, const double* C_k, const double* sz_k, const double* sy_k,
                                   const double* syy_k, int64_t n_k, double* Gc, double* Rc, double* vy, int E, int V,
                                   void* stream) {
  VLB_REQUIRE(G_k && C_k && sz_k && sy_k && syy_k && Gc && Rc && vy, "ridge_cv_center: null argument");
  VLB_REQUIRE(E >= 1 && V >= 1 && n_k >= 1, "ridge_cv_center: bad shape E=%d V=%d n_k=%lld", E, V, (long long)n_k);
  const double inv_n = 1.0 / (double)n_k;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ridge_form_a_kernel, dim3((E + 255) / 256, E), dim3(256), 0, st, G_k, sz_k, Gc, E, inv_n, 0.0);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(ridge_form_r_kernel, dim3((E + 255) / 256, V), dim3(256), 0, st, C_k, sz_k, sy_k, Rc, E, inv_n);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(cv_vy_kernel, dim3((V + 255) / 256), dim3(256), 0, st, syy_k, sy_k, vy, V, inv_n);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

extern "C" int64_t vlb_ridge_cv_ws_doubles(int E, int V) {
  if (E < 1 || V < 1) return 0;
  return (int64_t)V * ((E + TS - 1) / TS);
}

extern "C" int vlb_ridge_cv_score(const double* X, const double* Gc, const double* Rc, const double* vy, double* ws, double* r_out,
                                  const int* info, int E, int V, void* stream) {
  VLB_REQUIRE(X && Gc && Rc && vy && ws && r_out && info, "ridge_cv_score: null argument");
  VLB_REQUIRE(E >= 1 && V >= 1, "ridge_cv_score: bad shape E=%d V=%d", E, V);
  hipStream_t st = as_stream(stream);
  const int nct = (E + TS - 1) / TS;
  hipLaunchKernelGGL(cv_quad_tile_kernel, tiles(V, E), dim3(256), 0, st, X, Gc, ws, E, V, info);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(cv_finish_kernel, dim3(V), dim3(256), 0, st, X, Rc, vy, ws, r_out, E, nct, info);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}

// vlb_ridge_cv_score's two launches; r_out[v] is written only where choice[v] == want
extern "C" int vlb_ridge_cv_score_rows(const double* X, const double* Gc, const double* Rc, const double* vy, double* ws,
                                       double* r_out, const int* info, int E, int V, const int* choice, int want, void* stream) {
  VLB_REQUIRE(X && Gc && Rc && vy && ws && r_out && info && choice, "ridge_cv_score_rows: null argument");
  VLB_REQUIRE(E >= 1 && V >= 1, "ridge_cv_score_rows: bad shape E=%d V=%d", E, V);
  VLB_REQUIRE(want >= 0, "ridge_cv_score_rows: want=%d is negative", want);
  hipStream_t st = as_stream(stream);
  const int nct = (E + TS - 1) / TS;
  hipLaunchKernelGGL(cv_quad_tile_kernel, tiles(V, E), dim3(256), 0, st, X, Gc, ws, E, V, info);
  VLB_LAUNCH_CHECK();
  hipLaunchKernelGGL(cv_finish_rows_kernel, dim3(V), dim3(256), 0, st, X, Rc, vy, ws, r_out, E, nct, info, choice, want);
  VLB_LAUNCH_CHECK();
  return VLB_OK;
}
