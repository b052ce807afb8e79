// aux_kernels.hip -- small device helpers around the hot path: state initialisation, model
// export, and the plant simulators used to close the loop on the device.
//   Duffing   x1' = x2, x2' = -0.5 x2 + x1 - x1^3 + u            duffing.py:255
//             after step 100: x2' = -5 x2 + 2 x1 - 0.5 x1^3 + u   duffing.py:991-992
//   Van der Pol  x1' = 2 x2, x2' = 2 x2 - 10 x1^2 x2 - 0.8 x1 + u vanderpol_RBF.py:113
//             after step 100: x1' = x2, x2' = -3 x2 - 10 x1^2 x2 - 3 x1 + u  vanderpol.py:923-931
//   RK4, h = 0.05                                                duffing.py:256-261
#include <cstdio>
#include "kernels.h"
#include <cstdlib>
#include "plant_device.h"
#include "state_rows.h"

namespace kmpc {

const char* dbg_env(const char* name) {
  static const bool on = getenv("KMPC_DEBUG") != nullptr;
  if (!on) {
    // a measurement switch in the environment of a process that has not asked for them: say so once instead of silently running the
    // default path (a script that compares "with" and "without" would otherwise compare the default with itself)
    static bool warned = false;
    if (!warned && getenv(name)) {
      warned = true;
      fprintf(stderr, "libkoopmpc: %s is set but ignored -- the KMPC_* measurement switches are read only when KMPC_DEBUG is set\n", name);
    }
    return nullptr;
  }
  return getenv(name);
}


template <typename T> __global__ __launch_bounds__(256) void plant_kernel(const PlantArgs<T> a) {
  const int B = a.B;
  for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
    T x1 = a.X[b], x2 = a.X[(size_t)B + b];
    plant_apply<T>(a.plant, a.switched, a.h, x1, x2, a.U[b]);
    a.X[b] = x1;
    a.X[(size_t)B + b] = x2;
  }
}

template <typename T> hipError_t launch_plant(const PlantArgs<T>& a, hipStream_t s) {
  if (a.B <= 0) return hipSuccess;
  int grid = (a.B + 255) / 256;
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL((plant_kernel<T>), dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

// P = P0 I, bar_Q = Q0 I, K = 0, C = 0 for every trajectory   (duffing.py:927-930, 944-946)
template <typename T>
__global__ __launch_bounds__(256) void fill_state_kernel(T* P, long strideP, int p, T P0, T* Qb, long strideQ, int L,
                                                         T Q0, T* K, long strideK, T* C, long strideC, int n) {
  const int b = blockIdx.x;
  T* Pb = P + (size_t)b * strideP;
  for (int e = threadIdx.x; e < (int)strideP; e += blockDim.x) Pb[e] = (e < p * p && e / p == e % p) ? P0 : T(0);
  T* Qq = Qb + (size_t)b * strideQ;
  for (int e = threadIdx.x; e < (int)strideQ; e += blockDim.x) Qq[e] = (e < L * L && e / L == e % L) ? Q0 : T(0);
  if (K) {
    T* Kb = K + (size_t)b * strideK;
    for (int e = threadIdx.x; e < (int)strideK; e += blockDim.x) Kb[e] = T(0);
  }
  if (C) {
    T* Cb = C + (size_t)b * strideC;
    for (int e = threadIdx.x; e < (int)strideC; e += blockDim.x) Cb[e] = T(0);
  }
}

template <typename T>
hipError_t launch_fill_state(T* P, long strideP, int p, T P0, T* Qb, long strideQ, int L, T Q0, T* K, long strideK,
                             T* C, long strideC, int n, int B, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL((fill_state_kernel<T>), dim3(B), dim3(256), 0, s, P, strideP, p, P0, Qb, strideQ, L, Q0, K,
                     strideK, C, strideC, n);
  return hipGetLastError();
}

// split K = [A B] (duffing.py:965-967) into dense per-trajectory blocks
template <typename T>
__global__ __launch_bounds__(256) void export_model_kernel(const T* K, long strideK, const T* C, long strideC, int n,
                                                           int L, T* A_out, T* B_out, T* C_out) {
  const int b = blockIdx.x, p = L + 1;
  const T* Kb = K + (size_t)b * strideK;
  if (A_out)
    for (int e = threadIdx.x; e < L * L; e += blockDim.x) A_out[(size_t)b * L * L + e] = Kb[(e / L) * p + (e % L)];
  if (B_out)
    for (int e = threadIdx.x; e < L; e += blockDim.x) B_out[(size_t)b * L + e] = Kb[e * p + L];
  if (C_out && C) {
    const T* Cb = C + (size_t)b * strideC;
    for (int e = threadIdx.x; e < n * L; e += blockDim.x) C_out[(size_t)b * n * L + e] = Cb[e];
  }
}

template <typename T> __global__ __launch_bounds__(64) void qp_value_kernel(const T* H, const T* f, const T* c, const T* U, int N, int B, T* fun) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const T* Hb = H + (size_t)b * N * N;
  T acc = c[b];
  for (int i = 0; i < N; ++i) {
    const T ui = U[(size_t)i * B + b];
    T hu = f[(size_t)b * N + i];
    for (int j = 0; j < N; ++j) hu += Hb[i * N + j] * U[(size_t)j * B + b];
    acc += ui * hu;
  }
  fun[b] = acc;
}
template <typename T> hipError_t launch_qp_value(const T* H, const T* f, const T* c, const T* U, int N, int B, T* fun, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL((qp_value_kernel<T>), dim3((B + 63) / 64), dim3(64), 0, s, H, f, c, U, N, B, fun);
  return hipGetLastError();
}

// the inverse of export_model_kernel: dense A, B, C blocks -> state layout (kmpc_mpc_solve)
template <typename T>
__global__ __launch_bounds__(256) void import_model_kernel(const T* A, const T* Bv, const T* C, int shared, int n, int L, T* K,
                                                           long strideK, T* Cs, long strideC) {
  const int b = blockIdx.x, p = L + 1;
  const size_t m = shared ? 0 : (size_t)b;
  T* Kb = K + (size_t)b * strideK;
  for (int e = threadIdx.x; e < L * p; e += blockDim.x) {
    const int r = e / p, c = e - r * p;
    Kb[e] = c < L ? A[m * L * L + (size_t)r * L + c] : Bv[m * L + r];
  }
  if (C && Cs) {
    T* Cb = Cs + (size_t)b * strideC;
    for (int e = threadIdx.x; e < n * L; e += blockDim.x) Cb[e] = C[m * n * L + e];
  }
}
template <typename T>
hipError_t launch_import_model(const T* A, const T* Bv, const T* C, int shared, int n, int L, int B, T* K, long strideK,
                               T* Cs, long strideC, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL((import_model_kernel<T>), dim3(B), dim3(256), 0, s, A, Bv, C, shared, n, L, K, strideK, Cs, strideC);
  return hipGetLastError();
}

// data_generate.py:17-79 on the device: one thread per trajectory walks its n_steps plant steps (sequential in
// time, parallel over trajectories) and leaves the transition pairs in the panels the offline fit reads
template <typename T>
__global__ __launch_bounds__(256) void datagen_kernel(int plant, T h, const T* X0, const T* U, int n_traj, int n_steps, T* X, T* Y) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_traj) return;
  const size_t M = (size_t)n_traj * n_steps;
  T x1 = X0[t], x2 = X0[(size_t)n_traj + t];
  for (int i = 0; i < n_steps; ++i) {
    const size_t c = (size_t)i * n_traj + t;
    X[c] = x1; X[M + c] = x2;
    plant_apply<T>(plant, 0, h, x1, x2, U[c]);
    Y[c] = x1; Y[M + c] = x2;
  }
}
template <typename T>
hipError_t launch_datagen(int plant, T h, const T* X0, const T* U, int n_traj, int n_steps, T* X, T* Y, hipStream_t s) {
  if (n_traj <= 0 || n_steps <= 0) return hipSuccess;
  hipLaunchKernelGGL((datagen_kernel<T>), dim3((n_traj + 255) / 256), dim3(256), 0, s, plant, h, X0, U, n_traj, n_steps, X, Y);
  return hipGetLastError();
}

template <typename T>
hipError_t launch_export_model(const T* K, long strideK, const T* C, long strideC, int n, int L, int B, T* A_out,
                               T* B_out, T* C_out, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL((export_model_kernel<T>), dim3(B), dim3(256), 0, s, K, strideK, C, strideC, n, L, A_out, B_out,
                     C_out);
  return hipGetLastError();
}

// dst[b*stride + e] = src[e]  (offline model handed to every trajectory, duffing.py:811-813)
template <typename T>
__global__ __launch_bounds__(256) void broadcast_kernel(T* dst, long stride, const T* src, int count) {
  T* d = dst + (size_t)blockIdx.x * stride;
  for (int e = threadIdx.x; e < count; e += blockDim.x) d[e] = src[e];
}
template <typename T> hipError_t launch_broadcast(T* dst, long stride, const T* src, int count, int B, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL((broadcast_kernel<T>), dim3(B), dim3(256), 0, s, dst, stride, src, count);
  return hipGetLastError();
}

// g <- a * g + d   (Gram accumulation with forgetting)
__global__ __launch_bounds__(256) void axpby_kernel(double* g, const double* d, double a, int count) {
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < count; e += gridDim.x * blockDim.x) g[e] = a * g[e] + d[e];
}
hipError_t launch_axpby(double* g, const double* d, double a, int count, hipStream_t s) {
  hipLaunchKernelGGL(axpby_kernel, dim3((count + 255) / 256), dim3(256), 0, s, g, d, a, count);
  return hipGetLastError();
}

#define INST(T)                                                                                                      \
  template hipError_t launch_plant<T>(const PlantArgs<T>&, hipStream_t);                                             \
  template hipError_t launch_fill_state<T>(T*, long, int, T, T*, long, int, T, T*, long, T*, long, int, int,        \
                                           hipStream_t);                                                             \
  template hipError_t launch_broadcast<T>(T*, long, const T*, int, int, hipStream_t);                                \
  template hipError_t launch_export_model<T>(const T*, long, const T*, long, int, int, int, T*, T*, T*, hipStream_t); \
  template hipError_t launch_import_model<T>(const T*, const T*, const T*, int, int, int, int, T*, long, T*, long,   \
                                             hipStream_t);                                                           \
  template hipError_t launch_datagen<T>(int, T, const T*, const T*, int, int, T*, T*, hipStream_t);                  \
  template hipError_t launch_qp_value<T>(const T*, const T*, const T*, const T*, int, int, T*, hipStream_t);
INST(float)
INST(double)

// ---------------------------------------------------------------------------------------
// dense state blocks <-> wave image of the register-state step (step_v2.h: V2Dims).  One workgroup per trajectory;
// the image is walked element by element (coalesced on the image side), padding elements are written as zero.
// ---------------------------------------------------------------------------------------
template <bool TO_IMAGE>
__global__ __launch_bounds__(256) void state_image_kernel(double* P, long sP, double* K, long sK, double* Q, long sQ, double* C, long sC,
                                                          int n, int L, double* img, long stride) {
  const V2Dims d(L, n);
  const int b = blockIdx.x, p = L + 1;
  double* const im = img + (size_t)b * stride;
  const long l2 = (long)d.cp * d.s2 * 2, tot = d.elems();
  for (long e = threadIdx.x; e < tot; e += blockDim.x) {
    const bool lay2 = e < l2;
    const long r = lay2 ? e : e - l2;
    const int S = lay2 ? d.s2 : d.s1;
    const int col = (int)(r / (2 * S)) * 2 + (int)(r & 1), slot = (int)((r >> 1) % S);
    double* src = nullptr;
    if (lay2) {
      if (slot < p) { if (col < p) src = P + (size_t)b * sP + (size_t)slot * p + col; }
      else if (col < L) src = Q + (size_t)b * sQ + (size_t)(slot - p) * L + col;
    } else {
      if (slot < L) { if (col < p) src = K + (size_t)b * sK + (size_t)slot * p + col; }
      else if (col < L && C) src = C + (size_t)b * sC + (size_t)(slot - L) * L + col;
    }
    if (TO_IMAGE) im[e] = src ? *src : 0.0;
    else if (src) *src = im[e];
  }
}
long state_image_elems(int L, int n) { return V2Dims(L, n).elems(); }
hipError_t launch_state_to_image(const double* P, long sP, const double* K, long sK, const double* Q, long sQ, const double* C, long sC,
                                 int n, int L, int B, double* img, long stride, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL((state_image_kernel<true>), dim3(B), dim3(256), 0, s, const_cast<double*>(P), sP, const_cast<double*>(K), sK,
                     const_cast<double*>(Q), sQ, const_cast<double*>(C), sC, n, L, img, stride);
  return hipGetLastError();
}
hipError_t launch_image_to_state(const double* img, long stride, int n, int L, int B, double* P, long sP, double* K, long sK,
                                 double* Q, long sQ, double* C, long sC, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL((state_image_kernel<false>), dim3(B), dim3(256), 0, s, P, sP, K, sK, Q, sQ, C, sC, n, L, const_cast<double*>(img), stride);
  return hipGetLastError();
}

// ---- diagnostics of one step's RLS update from the dense state blocks (RlsDiagArgs, kernels.h) ----------------------------------
// With lam = 1 the update is rank one -- [A B] += e g', C += e_c h' (duffing.py:927-953 in gain form) -- so the spectral norms the
// reference logs as A_error, B_error, C_error (duffing.py:985-990) are |e| |g[0:L]|, |e| |g[L]| and |e_c| |h|.  One wave per trajectory,
// launched in front of the step whose update it describes; every matrix is read once, a row at a time across the lanes.
__device__ __forceinline__ double diag_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
// y_r = sum_j M[r][j] v_j, r < rows, j < cols <= 128 (v_j in lane j & 63, register j >> 6); lane r & 63 keeps y_r in y[r >> 6]
__device__ __forceinline__ void diag_matvec(const double* M, int rows, int cols, int ld, double v0, double v1, int lane, double (&y)[2]) {
  y[0] = 0.0; y[1] = 0.0;
  for (int r = 0; r < rows; ++r) {
    const double* row = M + (size_t)r * ld;
    double s = lane < cols ? row[lane] * v0 : 0.0;
    if (lane + 64 < cols) s += row[lane + 64] * v1;
    s = diag_wave_sum(s);
    if ((r & 63) == lane) y[r >> 6] = s;
  }
}
__global__ __launch_bounds__(64) void rls_diag_kernel(const RlsDiagArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, L = a.L, p = L + 1, n = a.n, B = a.B;
  const double* const psn = a.psi_now + (size_t)b * L;
  if (a.Psi_row && lane < L) a.Psi_row[(size_t)lane * B + b] = psn[lane];
  double dA = 0.0, dB = 0.0, dC = 0.0;
  if (a.has_update && a.first_update) {
    // K_A = 0, bar_X = 0 (duffing.py:927-928, 944-945): the model in use was not the estimator's, the change has full rank
    dA = dB = dC = __builtin_nan("");
  } else if (a.has_update) {
    const double* const psp = a.psi_prev + (size_t)b * L;
    const double u = a.u_prev[b];
    const double psi0 = lane < L ? psp[lane] : 0.0;
    const double z0 = lane < L ? psi0 : (lane == L ? u : 0.0), z1 = lane + 64 == L ? u : 0.0;  // z = [psi; u], p <= 65 elements
    double pz[2], kz[2];
    diag_matvec(a.P + (size_t)b * a.strideP, p, p, p, z0, z1, lane, pz);
    const double d = 1.0 + diag_wave_sum(z0 * pz[0] + z1 * pz[1]);
    const double g0 = pz[0] / d, g1 = pz[1] / d;
    diag_matvec(a.K + (size_t)b * a.strideK, L, p, p, z0, z1, lane, kz);
    const double e = lane < L ? psn[lane] - kz[0] : 0.0;
    const double en = sqrt(diag_wave_sum(e * e));
    const double gn = sqrt(diag_wave_sum(lane < L ? g0 * g0 : 0.0));
    const double gL = L < 64 ? __shfl(g0, L, 64) : __shfl(g1, 0, 64);
    dA = en * gn;
    dB = en * fabs(gL);
    if (a.use_C) {
      double qp[2], cp[2];
      diag_matvec(a.Qb + (size_t)b * a.strideQ, L, L, L, psi0, 0.0, lane, qp);
      const double dc = 1.0 + diag_wave_sum(psi0 * qp[0]);
      const double h = qp[0] / dc;  // (0 in the lanes beyond L)
      diag_matvec(a.C + (size_t)b * a.strideC, n, L, L, psi0, 0.0, lane, cp);
      const double ec = lane < n ? a.x_now[(size_t)lane * B + b] - cp[0] : 0.0;
      dC = sqrt(diag_wave_sum(ec * ec)) * sqrt(diag_wave_sum(h * h));
    }
  }
  if (lane == 0) {
    if (a.dA_row) a.dA_row[b] = dA;
    if (a.dB_row) a.dB_row[b] = dB;
    if (a.dC_row) a.dC_row[b] = dC;
  }
}
hipError_t launch_rls_diag(const RlsDiagArgs& a, hipStream_t s) {
  if (a.B <= 0) return hipSuccess;
  if (a.L < 1 || a.L > 64 || a.n < 1 || a.n > 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(rls_diag_kernel, dim3(a.B), dim3(64), 0, s, a);
  return hipGetLastError();
}

template <typename S, typename D> __global__ __launch_bounds__(256) void cast_kernel(const S* __restrict__ src, D* __restrict__ dst, size_t count) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) dst[i] = (D)src[i];
}
template <typename S, typename D> hipError_t launch_cast(const S* src, D* dst, size_t count, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const size_t g = (count + 255) / 256;
  hipLaunchKernelGGL((cast_kernel<S, D>), dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, s, src, dst, count);
  return hipGetLastError();
}
template hipError_t launch_cast<float, double>(const float*, double*, size_t, hipStream_t);
template hipError_t launch_cast<double, float>(const double*, float*, size_t, hipStream_t);

// place_kernel: rank of every trajectory by last launch's solver work (descending, ties by index), then the card deal of RolloutArgs::perm.
// Round 6: a stable least-significant-digit radix sort by ONE workgroup, O(B), for batches beyond 16 384 -- rounds 4-5 compared every pair
// (O(B^2 / 16): 9 us at B = 4096, 62 us at 16 384) and had NO deal beyond; place_pairs_kernel below still serves B <= 16384.  The key is the work clipped to 12 bits and inverted (heavy first); three passes of four
// bits over ping-pong buffers of packed (key << 20 | index) words in global memory (L2-resident: B words); the elements start in index
// order and every pass is stable, so ties stay in index order: the result is a function of `work` alone (deterministic, as before).
// A pass: every thread counts the digits of its contiguous chunk (16 counters), the 16 x 1024 counts are scanned digit-major in LDS,
// every thread scatters its chunk in order.
constexpr int PLACE_T = 1024;
__global__ __launch_bounds__(PLACE_T) void place_kernel(const int32_t* __restrict__ work, int B, uint32_t* __restrict__ buf0, uint32_t* __restrict__ buf1,
                                                        int32_t* __restrict__ perm) {
  __shared__ int sCnt[16 * PLACE_T];   // [digit][thread]
  __shared__ int sPart[PLACE_T];
  const int t = threadIdx.x;
  const int C = (B + PLACE_T - 1) / PLACE_T, e0 = t * C, e1 = e0 + C < B ? e0 + C : B;
  for (int e = e0; e < e1; ++e) {
    int w = work[e];
    w = w < 0 ? 0 : (w > 4095 ? 4095 : w);
    buf0[e] = ((uint32_t)(4095 - w) << 20) | (uint32_t)e;
  }
  __syncthreads();
  uint32_t* src = buf0;
  uint32_t* dst = buf1;
  for (int pass = 0; pass < 3; ++pass) {
    const int sh = 20 + 4 * pass;
    int cnt[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) cnt[d] = 0;
    for (int e = e0; e < e1; ++e) {
      const int d = (src[e] >> sh) & 15;
#pragma unroll
      for (int dd = 0; dd < 16; ++dd) cnt[dd] += (dd == d) ? 1 : 0;  // (no dynamic register index)
    }
#pragma unroll
    for (int d = 0; d < 16; ++d) sCnt[d * PLACE_T + t] = cnt[d];
    __syncthreads();
    // exclusive scan of the 16 x 1024 counts in digit-major order: thread t owns entries 16 t .. 16 t + 15 of the flattened array
    int loc[16], sum = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) { loc[i] = sum; sum += sCnt[16 * t + i]; }
    // (1024 partial sums: inclusive scan inside each wave by shuffles, the sixteen wave totals through LDS)
    int inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int v = __shfl_up(inc, off, 64);
      if ((t & 63) >= off) inc += v;
    }
    if ((t & 63) == 63) sPart[t >> 6] = inc;
    __syncthreads();
    int wbase = 0;
    for (int wv2 = 0; wv2 < (t >> 6); ++wv2) wbase += sPart[wv2];
    const int base = wbase + inc - sum;  // exclusive
    __syncthreads();  // (sPart is rewritten by the next pass)
#pragma unroll
    for (int i = 0; i < 16; ++i) sCnt[16 * t + i] = base + loc[i];
    __syncthreads();
    int pos[16];
#pragma unroll
    for (int d = 0; d < 16; ++d) pos[d] = sCnt[d * PLACE_T + t];
    for (int e = e0; e < e1; ++e) {
      const uint32_t v = src[e];
      const int d = (v >> sh) & 15;
      int p = 0;
#pragma unroll
      for (int dd = 0; dd < 16; ++dd) { if (dd == d) { p = pos[dd]; pos[dd] += 1; } }
      dst[p] = v;
    }
    __threadfence_block();
    __syncthreads();
    uint32_t* const tmp = src; src = dst; dst = tmp;
  }
  // rank r -> slot of the card deal: stratum p = r / G goes to wave p of the G workgroups, in snake order
  const int G = B >> 4;
  for (int r = t; r < B; r += PLACE_T) {
    const int e = (int)(src[r] & 0xfffffu);
    const int p = r / G;
    int g = r - p * G;
    if (p & 1) g = G - 1 - g;
    // (stratum p -> wave p: age order.  Measured and dropped: strata 4-7 / 12-15 in reverse order so that the four SIMDs carry equal
    //  sums -- it undoes the gain: heavy solves on the OLDEST waves is what pays, profiles/r4_cfg2_placement_ab.txt)
    perm[g * 16 + p] = e;
  }
}
// The same table by comparing every pair (rounds 4-5): sixteen lanes share the scan of one element, B / 16 workgroups of 256 threads with
// the work panel in LDS (B <= 16384: 64 KB).  O(B^2 / 16), but spread over the whole chip: 8.7 us at B = 4096 and 62 us at 16 384, where
// the one-workgroup sort takes 28 and 93 us (three passes of global-memory round trips, strided chunk reads, barriers of sixteen waves:
// ~6 us per 1024 trajectories) -- it serves the batches up to 16 384, the sort everything beyond (where there was no deal at all).
__global__ __launch_bounds__(256) void place_pairs_kernel(const int32_t* __restrict__ work, int B, int32_t* __restrict__ perm) {
  extern __shared__ int32_t sW[];  // the whole work panel (B <= 16384: 64 KB): the scan reads it 16 times per workgroup
  for (int c = threadIdx.x; c < B; c += 256) { const int w = work[c]; sW[c] = w < 0 ? 0 : (w > 4095 ? 4095 : w); }  // (the sort's key)
  __syncthreads();
  const int e = blockIdx.x * 16 + (threadIdx.x >> 4), part = threadIdx.x & 15;
  const int we = e < B ? sW[e] : 0;
  int r = 0;
#pragma unroll 8
  for (int c = part; c < B; c += 16) {
    const int wc = sW[c];
    r += (wc > we || (wc == we && c < e)) ? 1 : 0;
  }
  r += __shfl_xor(r, 8, 64); r += __shfl_xor(r, 4, 64); r += __shfl_xor(r, 2, 64); r += __shfl_xor(r, 1, 64);
  if (part == 0 && e < B) {
    const int G = B >> 4, p = r / G;
    int g = r - p * G;
    if (p & 1) g = G - 1 - g;
    perm[g * 16 + p] = e;
  }
}
// scratch: 2 B words (the sort's buffers).  B a multiple of 16, at most 2^20 trajectories.
hipError_t launch_place(const int32_t* work, int B, int32_t* perm, uint32_t* scratch, hipStream_t s) {
  if (B <= 0 || (B & 15) || B > (1 << 20) || !scratch) return hipErrorInvalidValue;
  if (B <= 16384) {
    static bool configured_dev[16] = {};  // (function attributes are per device)
    bool& configured = configured_dev[device_slot()];
    if (!configured) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&place_pairs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
      configured = true;
    }
    hipLaunchKernelGGL(place_pairs_kernel, dim3(B / 16), dim3(256), (size_t)B * sizeof(int32_t), s, work, B, perm);
  } else {
    hipLaunchKernelGGL(place_kernel, dim3(1), dim3(PLACE_T), 0, s, work, B, scratch, scratch + B, perm);
  }
  return hipGetLastError();
}

// Row-major zero-padded weights (Mp x Hp) -> MFMA A-fragments [tile][k-step][lane]: lane l of tile t, k-step ks
// holds W[16 t + (l & 15)][4 ks + (l >> 4)], so a wave reads one fragment as 64 consecutive elements.
template <typename T> __global__ void pack_afrag_kernel(const T* src, int Mp, int Hp, int KS, T* dst) {
  const int total = (Mp / 16) * KS * 64;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int l = e & 63, ks = (e >> 6) % KS, t = (e >> 6) / KS;
    const int col = 4 * ks + (l >> 4);
    dst[e] = col < Hp ? src[(size_t)(16 * t + (l & 15)) * Hp + col] : T(0);
  }
}
template <typename T> hipError_t launch_pack_afrag(const T* src, int Mp, int Hp, int KS, T* dst, hipStream_t s) {
  const int total = (Mp / 16) * KS * 64;
  hipLaunchKernelGGL((pack_afrag_kernel<T>), dim3((total + 255) / 256), dim3(256), 0, s, src, Mp, Hp, KS, dst);
  return hipGetLastError();
}
template hipError_t launch_pack_afrag<float>(const float*, int, int, int, float*, hipStream_t);
template hipError_t launch_pack_afrag<double>(const double*, int, int, int, double*, hipStream_t);

// ---------------------------------------------------------------------------------------
// Packed rows of per-trajectory state (kmpc_state_pack / _unpack / _transfer; the row format: api.hip, the plan: state_rows.h).
// Pure data movement.  state_rows_check_kernel runs first and alone decides whether a call is valid; the copy kernels skip an index
// outside [0, B) on their own account all the same.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void state_rows_check_kernel(const int32_t* __restrict__ idx, int count, int B, int32_t* __restrict__ mark,
                                                               const char* __restrict__ rows, int elem, long row_elems, int flag_off,
                                                               int want_hp, int want_rf, int32_t* __restrict__ status) {
  // a flag element as an integer: 0 / 1, anything else -1
  auto flag_at = [&](long r, int k) -> int {
    const char* const e = rows + ((size_t)r * row_elems + flag_off + k) * elem;
    const double v = elem == 8 ? *reinterpret_cast<const double*>(e) : (double)*reinterpret_cast<const float*>(e);
    return v == 0.0 ? 0 : (v == 1.0 ? 1 : -1);
  };
  int hp0 = want_hp, rf0 = want_rf;
  if (rows && (want_hp < 0 || want_rf < 0)) { hp0 = flag_at(0, 0); rf0 = flag_at(0, 1); }  // (every thread reads row 0: one cached line)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) {
    const int b = idx ? idx[i] : (int)i;
    int bad = 0;
    if (b < 0 || b >= B) bad |= ROWS_BAD_RANGE;
    else if (mark && atomicAdd(&mark[b], 1) != 0) bad |= ROWS_BAD_DUP;
    if (rows) {
      const int hp = flag_at(i, 0), rf = flag_at(i, 1);
      if (hp < 0 || rf < 0) bad |= ROWS_BAD_FLAG_VALUE;
      else if (hp != hp0 || rf != rf0) bad |= ROWS_BAD_FLAG_MIXED;
      if (i == 0) bad |= (hp == 1 ? ROWS_ROW0_HAVE_PREV : 0) | (rf == 1 ? ROWS_ROW0_RLS_FRESH : 0);
    }
    if (bad) atomicOr(status, bad);
  }
}
hipError_t launch_state_rows_check(const int32_t* idx, int count, int B, int32_t* mark, const void* rows, const RowPlan& pl, int want_hp, int want_rf,
                                   int32_t* status, hipStream_t s) {
  if (count <= 0 || B <= 0 || !status) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t), s);
  if (e == hipSuccess && mark) e = hipMemsetAsync(mark, 0, sizeof(int32_t) * (size_t)B, s);
  if (e != hipSuccess) return e;
  const int grid = (count + 255) / 256;
  hipLaunchKernelGGL(state_rows_check_kernel, dim3(grid > 2048 ? 2048 : grid), dim3(256), 0, s, idx, count, B, mark, (const char*)rows, pl.elem,
                     (long)pl.row_elems, pl.flag_off, want_hp, want_rf, status);
  return hipGetLastError();
}

// len contiguous elements by the whole workgroup: 16-byte vectors where both sides are 16-byte aligned (every float64 segment: the
// even_up strides), 8-byte ones where both are 8-byte aligned (float32 segments), element by element otherwise; the tail likewise
typedef unsigned int rows_v4 __attribute__((ext_vector_type(4)));
typedef unsigned int rows_v2 __attribute__((ext_vector_type(2)));
template <typename T> __device__ __forceinline__ void rows_copy_contig(T* __restrict__ dst, const T* __restrict__ src, int len, int tid) {
  const uintptr_t a = (uintptr_t)dst | (uintptr_t)src;  // (wave-uniform: the trajectory index is)
  int done = 0;
  if ((a & 15) == 0) {
    constexpr int V = 16 / (int)sizeof(T);
    const int nv = len / V;
    for (int i = tid; i < nv; i += 256) reinterpret_cast<rows_v4*>(dst)[i] = reinterpret_cast<const rows_v4*>(src)[i];
    done = nv * V;
  } else if (sizeof(T) == 4 && (a & 7) == 0) {
    const int nv = len / 2;
    for (int i = tid; i < nv; i += 256) reinterpret_cast<rows_v2*>(dst)[i] = reinterpret_cast<const rows_v2*>(src)[i];
    done = nv * 2;
  }
  for (int i = done + tid; i < len; i += 256) dst[i] = src[i];
}
// one workgroup per packed row.  PACK: row <- trajectory, else trajectory <- row.
template <typename T, bool PACK>
__device__ __forceinline__ void state_rows_move(const RowPlan& pl, const int32_t* __restrict__ idx, int B, T* __restrict__ rows, T hp, T rf) {
  const int r = blockIdx.x, tid = threadIdx.x;
  const int b = __builtin_amdgcn_readfirstlane(idx ? idx[r] : r);  // read once, wave-uniform: every address below is base + lane offset
  if (b < 0 || b >= B) return;
  T* const row = rows + (size_t)r * pl.row_elems;
  const int lane = tid - 192;  // the last wave also takes the strided column, the scalars and the padding
  for (int k = 0; k < pl.nseg; ++k) {
    const RowSeg& g = pl.seg[k];
    T* const blk = reinterpret_cast<T*>(g.base) + (size_t)b * g.stride;
    T* const in_row = row + g.off;
    if (g.step == 1 && g.len > 1) {
      if (PACK) rows_copy_contig<T>(in_row, blk, g.len, tid);
      else rows_copy_contig<T>(blk, in_row, g.len, tid);
    } else if (lane >= 0) {
      for (int j = lane; j < g.len; j += 64) {
        if (PACK) in_row[j] = blk[(size_t)j * g.step];
        else blk[(size_t)j * g.step] = in_row[j];
      }
    }
  }
  if (PACK && lane >= 0)
    for (int j = pl.flag_off + lane; j < pl.row_elems; j += 64) row[j] = j == pl.flag_off ? hp : (j == pl.flag_off + 1 ? rf : T(0));
}
template <typename T> __global__ __launch_bounds__(256) void state_rows_gather_kernel(const RowPlan pl, const int32_t* __restrict__ idx, int B, T* __restrict__ rows, T hp, T rf) {
  state_rows_move<T, true>(pl, idx, B, rows, hp, rf);
}
template <typename T> __global__ __launch_bounds__(256) void state_rows_scatter_kernel(const RowPlan pl, const int32_t* __restrict__ idx, int B, const T* __restrict__ rows) {
  state_rows_move<T, false>(pl, idx, B, const_cast<T*>(rows), T(0), T(0));
}
static bool rows_plan_ok(const RowPlan& pl, size_t elem) {
  return pl.nseg >= 1 && pl.nseg <= RowPlan::kMaxSeg && (size_t)pl.elem == elem && pl.flag_off + 2 <= pl.row_elems;
}
template <typename T> hipError_t launch_state_rows_gather(const RowPlan& pl, const int32_t* idx, int count, int B, T* rows, int have_prev, int rls_fresh, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  if (!rows || B <= 0 || !rows_plan_ok(pl, sizeof(T))) return hipErrorInvalidValue;
  hipLaunchKernelGGL((state_rows_gather_kernel<T>), dim3(count), dim3(256), 0, s, pl, idx, B, rows, T(have_prev ? 1 : 0), T(rls_fresh ? 1 : 0));
  return hipGetLastError();
}
template <typename T> hipError_t launch_state_rows_scatter(const RowPlan& pl, const int32_t* idx, int count, int B, const T* rows, hipStream_t s) {
  if (count <= 0) return hipSuccess;
  if (!rows || B <= 0 || !rows_plan_ok(pl, sizeof(T))) return hipErrorInvalidValue;
  hipLaunchKernelGGL((state_rows_scatter_kernel<T>), dim3(count), dim3(256), 0, s, pl, idx, B, rows);
  return hipGetLastError();
}
template hipError_t launch_state_rows_gather<float>(const RowPlan&, const int32_t*, int, int, float*, int, int, hipStream_t);
template hipError_t launch_state_rows_gather<double>(const RowPlan&, const int32_t*, int, int, double*, int, int, hipStream_t);
template hipError_t launch_state_rows_scatter<float>(const RowPlan&, const int32_t*, int, int, const float*, hipStream_t);
template hipError_t launch_state_rows_scatter<double>(const RowPlan&, const int32_t*, int, int, const double*, hipStream_t);

}  // namespace kmpc
