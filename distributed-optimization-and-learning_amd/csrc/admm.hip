// admm.hip — the primal/dual family on the agent-major bank: the fused prox /
// ADMM gradient term + momentum SGD step, the dual update and its residuals,
// the least-squares client round of FedAvg / FedProx / FedADMM (one TERMS
// selector; alone, and fused with the server's ordered mean), the one-pass
// SCAFFOLD round beside them, and the ordered sum / mean.
//
// What the rounds share is stated once: the local-step lanes are F-generic
// (float, or f2 packed; an f4 column is two f2 halves), and the one-pass
// rounds have one host launch plan (launch_strips) and one set of shared
// argument rules (check_strip_round).  The column-strip walk itself is still
// written out in both one-pass kernels, admm_ls_round_mean_kernel and
// scaffold_ls_round_kernel: a shared device-side skeleton taking the step, the
// chain and the epilogue as callables did not reproduce their code (DESIGN.md,
// "One strip walk: tried, left out"), so a fix to the dead-lane rule or the
// prefetch pipeline is made in both.
//
// Dropped launch variant (the default's bits; code last present at 1a824fc):
//   DOL_ADMM_ROUND_THREADS: admm_ls_round_mean_kernel strips forced to 1024 / 256 / 64 lanes; at 8192 x 2^17
//     18.6 / 7.4 / 7.65 ms, and 5.15 for the two-kernel round (profiles/r06c_admm_narrow_ab.jsonl).
#include <algorithm>
#include <initializer_list>
#include <utility>

#include "dol_launch.h"

namespace {
constexpr int kThreads = 256;            // 4 waves of 64

// ----------------------------------------------------------------------------
// Fused prox / ADMM gradient term + momentum SGD.
// MODE: 0 = no momentum, 1 = momentum first step (buf = g'), 2 = momentum.
// ----------------------------------------------------------------------------
template <bool THETA, bool ALPHA, int MODE, bool WRITE_G, bool DUAL = false>
__device__ __forceinline__ void prox_sgd_lane(float& w, float& bf, float& g, float th, float& al,
                                              float rho, float neg_lr, float mom) {
  float gg = g;
  if constexpr (THETA) {
    float t = rho * (w - th);
    if constexpr (ALPHA) t = al + t;
    gg = gg + t;
  }
  if constexpr (WRITE_G) g = gg;
  float d = gg;
  if constexpr (MODE == 1) { bf = gg; d = gg; }
  if constexpr (MODE == 2) { bf = bf * mom + gg; d = bf; }
  w = __builtin_fmaf(neg_lr, d, w);
  if constexpr (DUAL) al = al + rho * (w - th);  // update_duals on the new w (DEC/clients.py:141-144)
}

template <typename V, bool THETA, bool ALPHA, int MODE, bool WRITE_G, bool DUAL = false>
__global__ __launch_bounds__(kThreads) void prox_sgd_kernel(
    float* __restrict__ W, int64_t ldw, float* __restrict__ B, int64_t ldb, float* __restrict__ G,
    int64_t ldg, const float* __restrict__ theta, float* __restrict__ A, int64_t lda,
    float rho, float neg_lr, float mom, int64_t c_off, int64_t ncols_v, int64_t n_col_tiles) {
  const int64_t blk = blockIdx.x;
  const int64_t agent = blk / n_col_tiles;
  const int64_t c = (blk % n_col_tiles) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  V* wp = reinterpret_cast<V*>(W + agent * ldw + c_off) + c;
  V* gp = reinterpret_cast<V*>(G + agent * ldg + c_off) + c;
  // every per-agent row is read and written once: nontemporal both ways (r05:
  // 100 x 1,663,370 0.83 vs 0.90 ms, 1024 x 2^20 4.67 vs 4.96 ms,
  // profiles/r05zzr_prox_sgd_nt_ab.jsonl); theta is shared by all agents: cached
  constexpr bool DOL_PROX_NT = true;
  V w = ldv<V, DOL_PROX_NT>(wp), g = ldv<V, DOL_PROX_NT>(gp);
  V bf{}, th{}, al{};
  if constexpr (MODE == 2) bf = ldv<V, DOL_PROX_NT>(reinterpret_cast<V*>(B + agent * ldb + c_off) + c);
  if constexpr (THETA) th = *(reinterpret_cast<const V*>(theta + c_off) + c);
  if constexpr (ALPHA) al = ldv<V, DOL_PROX_NT>(reinterpret_cast<const V*>(A + agent * lda + c_off) + c);
  if constexpr (Vec<V>::W == 1) {
    prox_sgd_lane<THETA, ALPHA, MODE, WRITE_G, DUAL>(w, bf, g, th, al, rho, neg_lr, mom);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float wj = w[j], bj = bf[j], gj = g[j], aj = al[j];
      prox_sgd_lane<THETA, ALPHA, MODE, WRITE_G, DUAL>(wj, bj, gj, th[j], aj, rho, neg_lr, mom);
      w[j] = wj;
      bf[j] = bj;
      g[j] = gj;
      al[j] = aj;
    }
  }
  stv<V, DOL_PROX_NT>(wp, w);
  if constexpr (WRITE_G) stv<V, DOL_PROX_NT>(gp, g);
  if constexpr (MODE != 0) stv<V, DOL_PROX_NT>(reinterpret_cast<V*>(B + agent * ldb + c_off) + c, bf);
  if constexpr (DUAL) stv<V, DOL_PROX_NT>(reinterpret_cast<V*>(A + agent * lda + c_off) + c, al);
}

// Gradient term alone: g += rho*(w - theta) (+ alpha), w untouched.
template <typename V, bool ALPHA>
__global__ __launch_bounds__(kThreads) void prox_grad_kernel(
    float* __restrict__ G, int64_t ldg, const float* __restrict__ W, int64_t ldw,
    const float* __restrict__ theta, const float* __restrict__ A, int64_t lda, float rho,
    int64_t c_off, int64_t ncols_v, int64_t n_col_tiles) {
  const int64_t blk = blockIdx.x;
  const int64_t agent = blk / n_col_tiles;
  const int64_t c = (blk % n_col_tiles) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  V* gp = reinterpret_cast<V*>(G + agent * ldg + c_off) + c;
  const V w = *(reinterpret_cast<const V*>(W + agent * ldw + c_off) + c);
  const V th = *(reinterpret_cast<const V*>(theta + c_off) + c);
  V t = rho * (w - th);
  if constexpr (ALPHA) t = *(reinterpret_cast<const V*>(A + agent * lda + c_off) + c) + t;
  *gp = *gp + t;
}

// ----------------------------------------------------------------------------
// ADMM dual update alpha += rho*(w - theta), with optional per-agent
// ||w-theta||^2 partials (fp64, fixed reduction tree -> deterministic).
// One block = kThreads lanes x kDualIters V-columns of one agent.
// ----------------------------------------------------------------------------
constexpr int kDualIters = 4;

template <int NT = kThreads>
__device__ __forceinline__ double block_sum_f64(double v, double* smem) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) smem[wid] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0) {
    for (int i = 0; i < NT / 64; ++i) s += smem[i];
  }
  return s;
}

__device__ __forceinline__ float dual_lane(float& a, float w, float th, float rho, double& r) {
  const float d = w - th;
  a = a + rho * d;
  r += double(d) * double(d);
  return d;
}

// VEC: columns [0, n4) as f4, then the (< 4) tail columns by the first
// lanes of the agent's last chunk; !VEC: all P columns scalar.
template <bool VEC, bool RESID>
__global__ __launch_bounds__(kThreads) void admm_dual_kernel(
    float* __restrict__ A, int64_t lda, const float* __restrict__ W, int64_t ldw,
    const float* __restrict__ theta, float rho, int64_t P, int64_t n_chunks,
    double* __restrict__ partial) {
  __shared__ double smem[kThreads / 64];
  const int64_t blk = blockIdx.x;
  const int64_t agent = blk / n_chunks;
  const int64_t chunk = blk % n_chunks;
  float* arow = A + agent * lda;
  const float* wrow = W + agent * ldw;
  double r = 0.0;
  if constexpr (VEC) {
    const int64_t n4 = P / 4;
#pragma unroll
    for (int it = 0; it < kDualIters; ++it) {
      const int64_t c = (chunk * kDualIters + it) * kThreads + threadIdx.x;
      if (c < n4) {
        // rows read / written once: nontemporal (r05: 100 x 1,663,370 0.378 vs
        // 0.395 ms, 1024 x 2^20 2.16 vs 2.37 ms, profiles/r05zzs_admm_dual_nt_ab.jsonl)
        constexpr bool DOL_DUAL_NT = true;
        f4* ap = reinterpret_cast<f4*>(arow) + c;
        const f4 w = ldv<f4, DOL_DUAL_NT>(reinterpret_cast<const f4*>(wrow) + c);
        const f4 th = reinterpret_cast<const f4*>(theta)[c];
        f4 a = ldv<f4, DOL_DUAL_NT>(ap);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float aj = a[j];
          dual_lane(aj, w[j], th[j], rho, r);
          a[j] = aj;
        }
        stv<f4, DOL_DUAL_NT>(ap, a);
      }
    }
    const int64_t tail = P - 4 * n4;
    if (chunk == n_chunks - 1 && threadIdx.x < tail) {
      const int64_t c = 4 * n4 + threadIdx.x;
      float a = arow[c];
      dual_lane(a, wrow[c], theta[c], rho, r);
      arow[c] = a;
    }
  } else {
#pragma unroll
    for (int it = 0; it < kDualIters; ++it) {
      const int64_t c = (chunk * kDualIters + it) * kThreads + threadIdx.x;
      if (c < P) {
        float a = arow[c];
        dual_lane(a, wrow[c], theta[c], rho, r);
        arow[c] = a;
      }
    }
  }
  if constexpr (RESID) {
    const double s = block_sum_f64(r, smem);
    if (threadIdx.x == 0) partial[agent * n_chunks + chunk] = s;
  }
}

// partial layout: [n_agents][n_chunks_total]; one block per agent, fixed order.
__global__ __launch_bounds__(kThreads) void resid_reduce_kernel(const double* __restrict__ partial,
                                                                int64_t n_chunks,
                                                                double* __restrict__ out) {
  __shared__ double smem[kThreads / 64];
  const int64_t agent = blockIdx.x;
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < n_chunks; i += kThreads) v += partial[agent * n_chunks + i];
  const double s = block_sum_f64(v, smem);
  if (threadIdx.x == 0) out[agent] = s;
}

// ----------------------------------------------------------------------------
// One FedADMM client round on the separable least-squares objective
// f_k(w) = 1/2 ||w - t_k||^2 (BASELINE config 4's primal/dual side), fused
// per sampled agent k (row a = agents[k]) — the reference's
// FedAdmm_Client.update_weights (DEC/clients.py:36-53) with the CNN gradient
// replaced by the exact least-squares one:
//   w = theta                                   (load_state_dict(theta), :37)
//   local_steps times:  g = fl(w - t)
//     g' = fl(g + fl(alpha + fl(rho * fl(w - theta))))        (:132-135)
//     SGD(lr, momentum).step(): buf = first ? g' : fl(fl(buf*mu) + g'); w = fma(-lr, buf, w)
//   alpha = fl(alpha + fl(rho * fl(w - theta)))  (update_duals, :141-144, pre-round theta)
// Streams t, alpha (, buf) in and w, alpha (, buf) out once; w is never read.
// RESID: fp64 per-block partials of ||w - theta||^2 and ||alpha||^2 (fixed
// reduction tree, deterministic), as admm_dual_kernel.
// ----------------------------------------------------------------------------
// TERMS selects the algorithm's gradient term (DOL_FED_AVG / _PROX / _ADMM), the
// three of one Server.run (DEC/servers.py:50-81):
//   0 FedAvg   g' = g                                  (DEC/clients.py:85-95)
//   1 FedProx  g' = fl(g + fl(rho * fl(w - theta)))    (:101-115)
//   2 FedADMM  the above, dual ascent included          (:125-144)
// update_duals is a no-op for 0 and 1 (:58-59): a and ra are then not touched.
// F is float or f2: two columns at once in packed fp32 (v_pk_add / v_pk_mul /
// v_pk_fma_f32 on gfx950, each an IEEE operation per half), the same rounding
// per element.  At 10 local steps the round runs ~70 fp32 ops per element:
// unpacked that is ~60 % of the HBM time in VALU issue.
typedef float f2 __attribute__((ext_vector_type(2)));
template <typename F> __device__ __forceinline__ F splat(float s) {
  if constexpr (std::is_same<F, float>::value) return s;
  else return F{s, s};
}
// the product of two floats is exact in double, so fma == the reference's
// separately rounded r + v*v, one instruction fewer
__device__ __forceinline__ void sq_acc(float v, double& r) { r = __builtin_fma(double(v), double(v), r); }
__device__ __forceinline__ void sq_acc(f2 v, double& r) {
  sq_acc(v.x, r);
  sq_acc(v.y, r);
}
// an f4 column runs as two packed halves (v.xy, v.zw); join() repacks them
__device__ __forceinline__ f4 join(f2 lo, f2 hi) { return f4{lo.x, lo.y, hi.x, hi.y}; }

template <bool MOM, int TERMS, typename F>
__device__ __forceinline__ void fed_ls_lane(F& w, F& b, F& a, F t, F th, float rho, float neg_lr, float mom, int steps,
                                            bool first, double& rw, double& ra) {
  const F rho_ = splat<F>(rho), nlr = splat<F>(neg_lr), mu = splat<F>(mom);
  w = th;
  for (int k = 0; k < steps; ++k) {
    const F g = w - t;
    F gg = g;
    if constexpr (TERMS == 2) gg = g + (a + rho_ * (w - th));
    if constexpr (TERMS == 1) gg = g + rho_ * (w - th);
    F d = gg;
    if constexpr (MOM) {
      b = (first && k == 0) ? gg : b * mu + gg;
      d = b;
    }
    w = __builtin_elementwise_fma(nlr, d, w);
  }
  const F dl = w - th;
  if constexpr (TERMS == 2) a = a + rho_ * dl;
  sq_acc(dl, rw);
  if constexpr (TERMS == 2) sq_acc(a, ra);
}
template <bool MOM, int TERMS>
__device__ __forceinline__ void fed_ls_lane(f4& w, f4& b, f4& a, f4 t, f4 th, float rho, float neg_lr, float mom,
                                            int steps, bool first, double& rw, double& ra) {
  f2 w0, w1, b0 = b.xy, b1 = b.zw, a0 = a.xy, a1 = a.zw;
  fed_ls_lane<MOM, TERMS>(w0, b0, a0, f2(t.xy), f2(th.xy), rho, neg_lr, mom, steps, first, rw, ra);
  fed_ls_lane<MOM, TERMS>(w1, b1, a1, f2(t.zw), f2(th.zw), rho, neg_lr, mom, steps, first, rw, ra);
  w = join(w0, w1);
  b = join(b0, b1);
  a = join(a0, a1);
}

// TERMS < 2 (FedAvg / FedProx): A is NULL, no dual row is read or written and
// no ||alpha||^2 partial is stored.
template <bool VEC, bool MOM, bool RESID, int TERMS = 2>
__global__ __launch_bounds__(kThreads) void admm_ls_round_kernel(
    float* __restrict__ W, int64_t ldw, float* __restrict__ B, int64_t ldb, float* __restrict__ A, int64_t lda,
    const float* __restrict__ T, int64_t ldt, const float* __restrict__ theta, const int32_t* __restrict__ agents,
    const int32_t* __restrict__ first, int64_t P, float rho, float neg_lr, float mom, int steps, int64_t n_chunks,
    double* __restrict__ partial) {
  __shared__ double smem[kThreads / 64];
  // agent-major blocks (consecutive blocks stream one row; a column-major order
  // put 2048 rows 4 MiB apart in flight at once and ran 1-2 % slower).  The
  // rows stream with nontemporal loads / stores so theta (4 MiB at 2^20, one
  // XCD's L2) stays resident for the next row instead of being evicted by them
  const int64_t blk = blockIdx.x;
  const int64_t k = blk / n_chunks;
  const int64_t chunk = blk % n_chunks;
  const int64_t a_row = agents ? agents[k] : k;
  const bool fst = first ? first[k] != 0 : false;
  float* wr = W + a_row * ldw;
  float* br = B + a_row * ldb;
  constexpr bool DUAL = TERMS == 2;
  float* ar = DUAL ? A + a_row * lda : nullptr;
  const float* tr = T + a_row * ldt;
  double rw = 0.0, ra = 0.0;
  auto one = [&](int64_t c) {
    float w, b = MOM ? br[c] : 0.0f, a = 0.0f;
    if constexpr (DUAL) a = ar[c];
    fed_ls_lane<MOM, TERMS>(w, b, a, tr[c], theta[c], rho, neg_lr, mom, steps, fst, rw, ra);
    wr[c] = w;
    if constexpr (DUAL) ar[c] = a;
    if constexpr (MOM) br[c] = b;
  };
  if constexpr (VEC) {
    const int64_t n4 = P / 4;
#pragma unroll
    for (int it = 0; it < kDualIters; ++it) {
      const int64_t c = (chunk * kDualIters + it) * kThreads + threadIdx.x;
      if (c < n4) {
        const f4 t = __builtin_nontemporal_load(reinterpret_cast<const f4*>(tr) + c);
        const f4 th = reinterpret_cast<const f4*>(theta)[c];
        f4 a = f4{0.f, 0.f, 0.f, 0.f};
        if constexpr (DUAL) a = __builtin_nontemporal_load(reinterpret_cast<const f4*>(ar) + c);
        f4 b = MOM ? __builtin_nontemporal_load(reinterpret_cast<const f4*>(br) + c) : f4{0.f, 0.f, 0.f, 0.f};
        f4 w;
        fed_ls_lane<MOM, TERMS>(w, b, a, t, th, rho, neg_lr, mom, steps, fst, rw, ra);
        __builtin_nontemporal_store(w, reinterpret_cast<f4*>(wr) + c);
        if constexpr (DUAL) __builtin_nontemporal_store(a, reinterpret_cast<f4*>(ar) + c);
        if constexpr (MOM) __builtin_nontemporal_store(b, reinterpret_cast<f4*>(br) + c);
      }
    }
    const int64_t tail = P - 4 * n4;
    if (chunk == n_chunks - 1 && threadIdx.x < tail) one(4 * n4 + threadIdx.x);
  } else {
#pragma unroll
    for (int it = 0; it < kDualIters; ++it) {
      const int64_t c = (chunk * kDualIters + it) * kThreads + threadIdx.x;
      if (c < P) one(c);
    }
  }
  if constexpr (RESID) {
    const double sw = block_sum_f64(rw, smem);
    double sa = 0.0;
    if constexpr (DUAL) {
      __syncthreads();
      sa = block_sum_f64(ra, smem);
    }
    if (threadIdx.x == 0) {
      partial[k * n_chunks + chunk] = sw;
      if constexpr (DUAL) partial[(gridDim.x / n_chunks + k) * n_chunks + chunk] = sa;
    }
  }
}

// ----------------------------------------------------------------------------
// Ordered sum / mean over gathered rows: acc = w[o0]; acc += w[o1]; ...
// Column-parallel; the row loop is unrolled so 8 row loads are in flight.
// ----------------------------------------------------------------------------
template <typename V>
__global__ __launch_bounds__(kThreads) void ordered_sum_kernel(
    const float* __restrict__ W, int64_t ldw, const int32_t* __restrict__ order, int m,
    int64_t c_off, int64_t ncols_v, const float* __restrict__ acc_in, float* __restrict__ out,
    float scale, int do_div) {
  const int64_t c = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  const V* wb = reinterpret_cast<const V*>(W + c_off) + c;
  const int64_t ldv = ldw / Vec<V>::W;
  V acc;
  int k;
  if (acc_in) {
    acc = *(reinterpret_cast<const V*>(acc_in + c_off) + c);
    k = 0;
  } else {
    acc = wb[int64_t(order[0]) * ldv];
    k = 1;
  }
  // the rows are read once: nontemporal loads (8192 x 2^20: 5.07-5.14 ms =
  // 6.77 TB/s vs 5.66-5.74 ms plain; 16 rows in flight instead of 8: no change;
  // profiles/r05zze_ordered_sum_ab.jsonl)
  for (; k + 8 <= m; k += 8) {
    V x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = __builtin_nontemporal_load(wb + int64_t(order[k + u]) * ldv);
#pragma unroll
    for (int u = 0; u < 8; ++u) acc = vadd(acc, x[u]);
  }
  for (; k < m; ++k) acc = vadd(acc, __builtin_nontemporal_load(wb + int64_t(order[k]) * ldv));
  if (do_div) acc = vdiv(acc, scale);
  *(reinterpret_cast<V*>(out + c_off) + c) = acc;
}

// ----------------------------------------------------------------------------
// The FedADMM client round fused with the server's ordered mean (one round of
// DEC/servers.py:50-81 on least squares: every sampled client's
// update_weights, DEC/clients.py:36-53, then average_weights, :42-48).
// Column-strip major: each lane owns one V-column and walks the m sampled
// agents in the given order, running fed_ls_lane on (agent, column) and
// chaining acc = w(first) ; acc = fl(acc + w) — the ordered_sum_kernel's
// association, so theta_next is the same bits as admm_ls_round_kernel +
// ordered_sum_kernel — while the w rows are still in registers: the separate
// mean read every sampled row back from HBM (34 GB at 8192 x 2^20, 15 % of the
// round's bytes).  theta is read once per lane, not once per (agent, column).
// The next agent group's t / alpha / buf loads are issued before the current
// group's steps (kRoundPF agents in flight per lane).
// RESID: fp64 per-lane sums over the agents of (w - theta)^2 and alpha^2, a
// fixed block tree, one partial per block; resid_reduce_kernel folds the
// blocks in a fixed order (the round's totals, not per agent).
// ----------------------------------------------------------------------------
constexpr int kRoundPF = 3;

__device__ __forceinline__ float ldnt(const float* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ f4 ldnt(const f4* p) { return __builtin_nontemporal_load(p); }
// nontemporal buffer store of lane value v at byte offset voff of the row at
// base (row-uniform resource); voff = kOOB drops it (still issued and counted)
__device__ __forceinline__ void st_row(float v, float* base, int64_t nbytes, uint32_t voff) {
  const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, static_cast<int>(nbytes), 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, voff, 0, 2);
}
__device__ __forceinline__ void st_row(f4 v, float* base, int64_t nbytes, uint32_t voff) {
  const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(base, 0, static_cast<int>(nbytes), 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), rs, voff, 0, 2);
}

// One prefetch group of the one-pass round: PF agents' target, dual and
// momentum rows in flight per lane.  Without duals (FedAvg / FedProx) it
// carries no a[].
template <typename V, int PF, bool DUAL> struct RoundGrp {
  V t[PF], a[PF], b[PF];
  int64_t row[PF];
};
template <typename V, int PF> struct RoundGrp<V, PF, false> {
  V t[PF], b[PF];
  int64_t row[PF];
};

// TERMS < 2 (FedAvg / FedProx): A is NULL; the group carries no dual rows, no
// dual row is loaded or stored and no ||alpha||^2 partial is written.
template <typename V, bool MOM, bool RESID, int NT, int TERMS = 2, int PF = kRoundPF>
__global__ __launch_bounds__(NT) void admm_ls_round_mean_kernel(
    float* __restrict__ W, int64_t ldw, float* __restrict__ B, int64_t ldb, float* __restrict__ A, int64_t lda,
    const float* __restrict__ T, int64_t ldt, const float* __restrict__ theta, const int32_t* __restrict__ agents,
    const int32_t* __restrict__ first, int m, int64_t c_off, int64_t ncols_v, float rho, float neg_lr, float mom,
    int steps, float* __restrict__ out, float scale, int do_div, double* __restrict__ partial, int64_t part_off,
    int64_t part_stride) {
  __shared__ double smem[NT / 64];
  const int64_t c = int64_t(blockIdx.x) * NT + threadIdx.x;
  const bool live = c < ncols_v;
  if (!RESID && !live) return;
  // dead lanes (RESID only) read the last real column and compute on it; their
  // stores are buffer stores pointed out of range (dropped, still counted, so
  // every lane issues the same memory ops and the loop's vmcnt waits stay
  // exact) and their residual terms are dropped
  const int64_t cc = live ? c : ncols_v - 1;
  const uint32_t voff = live ? uint32_t(c) * uint32_t(sizeof(V)) : kOOB;
  auto st = [&](V v, float* base, int64_t ld, int64_t row) {
    st_row(v, base + row * ld + c_off, std::min<int64_t>((ld - c_off) * 4, 0x7ffffff0), voff);
  };
  auto cptr = [&](const float* base, int64_t ld, int64_t row) {
    return reinterpret_cast<const V*>(base + row * ld + c_off) + cc;
  };
  auto row_of = [&](int k) -> int64_t {  // agent k's row; k past m: the last agent's (a harmless re-read)
    k = min(k, m - 1);
    return agents ? agents[k] : k;
  };
  const V th = *cptr(theta, 0, 0);
  V acc = vzero(th);
  double rw = 0.0, ra = 0.0;
  constexpr bool DUAL = TERMS == 2;
  using Grp = RoundGrp<V, PF, DUAL>;
  auto load = [&](Grp& g, int k0) {  // agents k0 .. k0 + PF - 1, unconditionally (rows clamped)
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      g.row[u] = row_of(k0 + u);
      g.t[u] = ldnt(cptr(T, ldt, g.row[u]));
      if constexpr (DUAL) g.a[u] = ldnt(cptr(A, lda, g.row[u]));
      if constexpr (MOM) g.b[u] = ldnt(cptr(B, ldb, g.row[u]));
    }
  };
  auto run = [&](Grp& g, int u, int k) {  // agent k = group slot u: its steps, stores, and the chain
    const bool fst = first ? first[k] != 0 : false;
    V w, bu = MOM ? g.b[u] : vzero(th), au = vzero(th);
    if constexpr (DUAL) au = g.a[u];
    double rwu = 0.0, rau = 0.0;
    fed_ls_lane<MOM, TERMS>(w, bu, au, g.t[u], th, rho, neg_lr, mom, steps, fst, rwu, rau);
    st(w, W, ldw, g.row[u]);
    if constexpr (DUAL) st(au, A, lda, g.row[u]);
    if constexpr (MOM) st(bu, B, ldb, g.row[u]);
    rw += live ? rwu : 0.0;
    ra += live ? rau : 0.0;
    acc = k == 0 ? w : vadd(acc, w);
  };
  const int ng = (m + PF - 1) / PF;  // groups; all but the last are full
  Grp nxt, cur;
  load(nxt, 0);
  for (int gi = 0; gi + 1 < ng; ++gi) {  // straight-line body: the same memory ops every trip
    cur = nxt;
    load(nxt, (gi + 1) * PF);      // the next group's loads fly during this group's steps
#pragma unroll
    for (int u = 0; u < PF; ++u) run(cur, u, gi * PF + u);
  }
#pragma unroll
  for (int u = 0; u < PF; ++u) {   // the last group (maybe partial)
    const int k = (ng - 1) * PF + u;
    if (k < m) run(nxt, u, k);
  }
  if (live) {
    if (do_div) acc = vdiv(acc, scale);
    *(reinterpret_cast<V*>(out + c_off) + c) = acc;
  }
  if constexpr (RESID) {
    const double sw = block_sum_f64<NT>(rw, smem);
    double sa = 0.0;
    if constexpr (DUAL) {
      __syncthreads();
      sa = block_sum_f64<NT>(ra, smem);
    }
    if (threadIdx.x == 0) {
      partial[part_off + blockIdx.x] = sw;
      if constexpr (DUAL) partial[part_stride + part_off + blockIdx.x] = sa;
    }
  }
}

// ----------------------------------------------------------------------------
// One SCAFFOLD server round on least squares in one pass: the client of the
// reference's sketch (DEC/clients.py:146-170, commented out there) and the
// server step of Karimireddy et al. 2020, Algorithm 1, on the column-strip
// skeleton of admm_ls_round_mean_kernel (a sibling kernel, so none of that
// template's instantiations moves).  Per sampled agent k (row a) and column:
//   w = theta
//   local_steps times:  g = fl(w - t_a);  g' = fl(fl(g + c) - c_a)       (:155)
//     momentum SGD as fed_ls_lane
//   dl   = fl(w - theta)                                                  (:162)
//   c_a' = fl(fl(c_a - c) - fl(dl * inv))   inv = 1 / (local_steps * lr)  (:165)
//   dc   = fl(c_a' - c_a)                                                 (:167)
//   acc_w = k == 0 ? dl : fl(acc_w + dl);  acc_c = k == 0 ? dc : fl(acc_c + dc)
// and once per column after the last agent
//   theta_out = fl(theta + fl(global_lr * fl(acc_w / scale_w)))
//   c_out     = fl(c + fl(acc_c / scale_c))
// The control variates c_a ride in the group's dual row slot; c is read once
// per lane like theta.  RESID: (dl^2, c_a'^2) summed as the FedADMM round's.
// F is float or f2 (packed, an IEEE operation per half).
// ----------------------------------------------------------------------------
template <bool MOM, typename F>
__device__ __forceinline__ void scaffold_ls_lane(F& w, F& b, F& ca, F& dl, F& dc, F t, F th, F c, float neg_lr,
                                                 float mom, float inv, int steps, bool first, double& rw, double& ra) {
  const F nlr = splat<F>(neg_lr), mu = splat<F>(mom);
  w = th;
  for (int k = 0; k < steps; ++k) {
    const F g = w - t;
    const F gg = (g + c) - ca;
    F d = gg;
    if constexpr (MOM) {
      b = (first && k == 0) ? gg : b * mu + gg;
      d = b;
    }
    w = __builtin_elementwise_fma(nlr, d, w);
  }
  dl = w - th;
  const F cn = (ca - c) - dl * splat<F>(inv);
  dc = cn - ca;
  ca = cn;
  sq_acc(dl, rw);
  sq_acc(cn, ra);
}
// f4 = two packed halves
template <bool MOM>
__device__ __forceinline__ void scaffold_ls_lane(f4& w, f4& b, f4& ca, f4& dl, f4& dc, f4 t, f4 th, f4 c, float neg_lr,
                                                 float mom, float inv, int steps, bool first, double& rw, double& ra) {
  f2 w0, w1, b0 = b.xy, b1 = b.zw, a0 = ca.xy, a1 = ca.zw, l0, l1, d0, d1;
  scaffold_ls_lane<MOM>(w0, b0, a0, l0, d0, f2(t.xy), f2(th.xy), f2(c.xy), neg_lr, mom, inv, steps, first, rw, ra);
  scaffold_ls_lane<MOM>(w1, b1, a1, l1, d1, f2(t.zw), f2(th.zw), f2(c.zw), neg_lr, mom, inv, steps, first, rw, ra);
  w = join(w0, w1);
  b = join(b0, b1);
  ca = join(a0, a1);
  dl = join(l0, l1);
  dc = join(d0, d1);
}
__device__ __forceinline__ float vscale(float a, float s) { return a * s; }
__device__ __forceinline__ f4 vscale(f4 a, float s) { return f4{a.x * s, a.y * s, a.z * s, a.w * s}; }

template <typename V, bool MOM, bool RESID, int NT, int PF = kRoundPF>
__global__ __launch_bounds__(NT) void scaffold_ls_round_kernel(
    float* __restrict__ W, int64_t ldw, float* __restrict__ B, int64_t ldb, float* __restrict__ CI, int64_t ldc,
    const float* __restrict__ T, int64_t ldt, const float* theta, const float* cglob,
    const int32_t* __restrict__ agents, const int32_t* __restrict__ first, int m, int64_t c_off, int64_t ncols_v,
    float neg_lr, float mom, int steps, float inv, float global_lr, float* theta_out, float scale_w, float* c_out,
    float scale_c, double* __restrict__ partial, int64_t part_off, int64_t part_stride) {
  __shared__ double smem[NT / 64];
  const int64_t c = int64_t(blockIdx.x) * NT + threadIdx.x;
  const bool live = c < ncols_v;
  if (!RESID && !live) return;
  // dead lanes (RESID only): as admm_ls_round_mean_kernel, they compute on the
  // last real column, their row stores go out of range and their sums are dropped
  const int64_t cc = live ? c : ncols_v - 1;
  const uint32_t voff = live ? uint32_t(c) * uint32_t(sizeof(V)) : kOOB;
  auto st = [&](V v, float* base, int64_t ld, int64_t row) {
    st_row(v, base + row * ld + c_off, std::min<int64_t>((ld - c_off) * 4, 0x7ffffff0), voff);
  };
  auto cptr = [&](const float* base, int64_t ld, int64_t row) {
    return reinterpret_cast<const V*>(base + row * ld + c_off) + cc;
  };
  auto row_of = [&](int k) -> int64_t {  // agent k's row; k past m: the last agent's (a harmless re-read)
    k = min(k, m - 1);
    return agents ? agents[k] : k;
  };
  // theta_out may be theta and c_out may be c: each lane reads its column here and writes it last
  const V th = *cptr(theta, 0, 0);
  const V cg = *cptr(cglob, 0, 0);
  V acc_w = vzero(th), acc_c = vzero(th);
  double rw = 0.0, ra = 0.0;
  using Grp = RoundGrp<V, PF, true>;  // a[] carries the control variates c_a
  auto load = [&](Grp& g, int k0) {  // agents k0 .. k0 + PF - 1, unconditionally (rows clamped)
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      g.row[u] = row_of(k0 + u);
      g.t[u] = ldnt(cptr(T, ldt, g.row[u]));
      g.a[u] = ldnt(cptr(CI, ldc, g.row[u]));
      if constexpr (MOM) g.b[u] = ldnt(cptr(B, ldb, g.row[u]));
    }
  };
  auto run = [&](Grp& g, int u, int k) {  // agent k = group slot u: its steps, stores, and the two chains
    const bool fst = first ? first[k] != 0 : false;
    V w, dl, dc, bu = MOM ? g.b[u] : vzero(th), au = g.a[u];
    double rwu = 0.0, rau = 0.0;
    scaffold_ls_lane<MOM>(w, bu, au, dl, dc, g.t[u], th, cg, neg_lr, mom, inv, steps, fst, rwu, rau);
    st(w, W, ldw, g.row[u]);
    st(au, CI, ldc, g.row[u]);
    if constexpr (MOM) st(bu, B, ldb, g.row[u]);
    rw += live ? rwu : 0.0;
    ra += live ? rau : 0.0;
    acc_w = k == 0 ? dl : vadd(acc_w, dl);
    acc_c = k == 0 ? dc : vadd(acc_c, dc);
  };
  const int ng = (m + PF - 1) / PF;  // groups; all but the last are full
  Grp nxt, cur;
  load(nxt, 0);
  for (int gi = 0; gi + 1 < ng; ++gi) {  // straight-line body: the same memory ops every trip
    cur = nxt;
    load(nxt, (gi + 1) * PF);      // the next group's loads fly during this group's steps
#pragma unroll
    for (int u = 0; u < PF; ++u) run(cur, u, gi * PF + u);
  }
#pragma unroll
  for (int u = 0; u < PF; ++u) {   // the last group (maybe partial)
    const int k = (ng - 1) * PF + u;
    if (k < m) run(nxt, u, k);
  }
  if (live) {
    *(reinterpret_cast<V*>(theta_out + c_off) + c) = vadd(th, vscale(vdiv(acc_w, scale_w), global_lr));
    *(reinterpret_cast<V*>(c_out + c_off) + c) = vadd(cg, vdiv(acc_c, scale_c));
  }
  if constexpr (RESID) {
    const double sw = block_sum_f64<NT>(rw, smem);
    __syncthreads();
    const double sa = block_sum_f64<NT>(ra, smem);
    if (threadIdx.x == 0) {
      partial[part_off + blockIdx.x] = sw;
      partial[part_stride + part_off + blockIdx.x] = sa;
    }
  }
}

// Chunks per row of the per-row kernels (admm_dual_kernel, admm_ls_round_kernel:
// kThreads x kDualIters V-columns a block); 0: too many blocks for one launch.
int64_t row_chunks(int64_t P, bool vec, int64_t rows) {
  const int64_t per_block = int64_t(kThreads) * kDualIters;
  const int64_t chunks = vec ? std::max<int64_t>(1, cdiv(P / 4, per_block)) : cdiv(P, per_block);
  return mul_sat(chunks, rows) > kMaxBlocks ? 0 : chunks;
}

// The argument rules the one-pass rounds share, after each round's own.
// m_why: why there must be a first sampled client; ld_short: some row matrix
// in use has ld < P.
int check_strip_round(const char* nm, int32_t m, const char* m_why, int64_t P, bool ld_short,
                      const double* resid_total, const void* work) {
  if (m < 1) return fail(DOL_EINVAL, "%s: m must be >= 1 (%s)", nm, m_why);
  if (resid_total && !work && P > 0) return fail(DOL_EINVAL, "%s: resid_total needs a workspace", nm);
  if (ld_short) return fail(DOL_EINVAL, "%s: ld < P", nm);
  if (P > (int64_t(1) << 29) - 16) return fail(DOL_EINVAL, "%s: P >= 2^29 (row offsets are 32-bit buffer offsets)", nm);
  return DOL_OK;
}

// One launch of a one-pass round: `blocks` strips of nt lanes over the ncols
// V-columns at c_off, their residual partials at part_off of [2][part_stride].
struct Strip {
  int nt;
  int64_t c_off, ncols, blocks;
  double* partial;
  int64_t part_off, part_stride;
};

// The launch plan of the one-pass rounds: columns [0, n4) as f4 where every
// (pointer, ld) of `rows` allows it, the rest scalar, one launch(V{}, Strip)
// each, then the fixed-order fold of the block partials into the n_totals
// doubles of resid_total (if asked for).
template <typename Launch>
void launch_strips(int64_t P, std::initializer_list<std::pair<const void*, int64_t>> rows, double* resid_total,
                   int n_totals, void* work, hipStream_t s, Launch launch) {
  bool vec_ok = true;
  for (const auto& r : rows) vec_ok = vec_ok && row_vec_ok(r.first, r.second);
  const ColSplit cs = split_cols(P, vec_ok);
  // column strip per workgroup: 1024 lanes (16 KiB of each row per workgroup,
  // one workgroup per CU at 2^20 columns).  Narrower blocks (fewer than 1024
  // lanes per CU) take 256-lane strips: the strips are the only parallelism
  // (the sum over agents is sequential per column).  At 8192 x 2^17 (a
  // column-sharded rank's block at 8 ranks): 18.6 ms with 1024-lane strips,
  // 7.4 with 256, 7.65 with one-wave strips and 8 agents in flight -- and 5.15
  // for the two-kernel round (row-major client round + ordered sum), which
  // SeparableADMM(shard="columns") takes there (profiles/r06c_admm_narrow_ab.jsonl).
  const int n_cu = n_cus() > 0 ? n_cus() : 256;
  const int64_t lanes = std::max<int64_t>(cs.n4, cs.tail);
  const int nt = lanes >= int64_t(1024) * n_cu ? 1024 : 256;
  const int64_t nb4 = cdiv(cs.n4, nt), nbt = cdiv(cs.tail, nt);
  const int64_t nb = nb4 + nbt;
  double* partial = static_cast<double*>(work);
  if (cs.n4 > 0) launch(f4{}, Strip{nt, 0, cs.n4, nb4, partial, 0, nb});
  if (cs.tail > 0) launch(float{}, Strip{nt, cs.n4 * 4, cs.tail, nbt, partial, nb4, nb});
  if (resid_total) hipLaunchKernelGGL(resid_reduce_kernel, dim3(n_totals), dim3(kThreads), 0, s, partial, nb, resid_total);
}

// The least-squares client round of the three algorithms; nm names the entry
// point in the messages.  alg == DOL_FED_ADMM is dol_admm_ls_round_f32 as ever.
int fed_ls_round(const char* nm, float* w, int64_t ldw, float* buf, int64_t ldb, float* alpha, int64_t lda,
                 const float* target, int64_t ldt, const float* theta, const int32_t* agents, const int32_t* first,
                 int32_t m, int64_t P, int32_t alg, float rho, float lr, float momentum, int32_t local_steps,
                 double* resid_sq, double* alpha_sq, void* work, hipStream_t s) {
  if (alg < DOL_FED_AVG || alg > DOL_FED_ADMM) return fail(DOL_EINVAL, "%s: algorithm must be 0 (FedAvg), 1 (FedProx) or 2 (FedADMM)", nm);
  const bool dual = alg == DOL_FED_ADMM;
  if (!dual) {
    if (alpha) return fail(DOL_EINVAL, "%s: FedAvg / FedProx have no duals (alpha must be NULL)", nm);
    if (alpha_sq) return fail(DOL_EINVAL, "%s: FedAvg / FedProx have no duals (alpha_sq must be NULL)", nm);
    lda = 0;
  }
  DOL_DIMS_OK(nm, ldw, ldb, lda, ldt, P);
  const bool mom = momentum != 0.0f;
  DOL_CHECKED(check_rows(nm, m < 0 || P < 0 || local_steps < 0, m == 0,
                         P > 0 && (!w || (dual && !alpha) || !target || !theta || (mom && !buf)), false, false));
  if (dual && (resid_sq == nullptr) != (alpha_sq == nullptr)) return fail(DOL_EINVAL, "%s: pass both residual outputs or neither", nm);
  if (resid_sq && !work && P > 0) return fail(DOL_EINVAL, "%s: residuals need a workspace", nm);
  if (ldw < P || (dual && lda < P) || ldt < P || (mom && ldb < P)) return fail(DOL_EINVAL, "%s: ld < P", nm);
  if (P == 0) {
    if (resid_sq) (void)hipMemsetAsync(resid_sq, 0, sizeof(double) * m, s);
    if (alpha_sq) (void)hipMemsetAsync(alpha_sq, 0, sizeof(double) * m, s);
    return check_launch(nm);
  }
  const bool vec = row_vec_ok(w, ldw) && row_vec_ok(alpha, lda) && row_vec_ok(target, ldt) && row_vec_ok(theta, 0) &&
                   (!mom || row_vec_ok(buf, ldb));
  const int64_t chunks = row_chunks(P, vec, m);
  if (!chunks) return fail(DOL_EINVAL, "%s: problem too large", nm);
  double* partial = static_cast<double*>(work);
  const dim3 grid(static_cast<unsigned>(chunks * m));
  dispatch([&](auto vc, auto mc, auto rc, auto tc) {
    hipLaunchKernelGGL((admm_ls_round_kernel<decltype(vc)::value, decltype(mc)::value, decltype(rc)::value,
                                             decltype(tc)::value>),
                       grid, dim3(kThreads), 0, s, w, ldw, buf, ldb, alpha, lda, target, ldt, theta, agents, first, P,
                       rho, -lr, momentum, local_steps, chunks, partial);
  }, Bool{vec}, Bool{mom}, Bool{resid_sq != nullptr}, Ints<0, 1, 2>{alg});
  if (resid_sq) hipLaunchKernelGGL(resid_reduce_kernel, dim3(m), dim3(kThreads), 0, s, partial, chunks, resid_sq);
  if (alpha_sq)
    hipLaunchKernelGGL(resid_reduce_kernel, dim3(m), dim3(kThreads), 0, s, partial + int64_t(m) * chunks, chunks,
                       alpha_sq);
  return check_launch(nm);
}

// The same fused with the server's ordered average (dol_admm_ls_round_mean_f32 for alg == DOL_FED_ADMM).
int fed_ls_round_mean(const char* nm, float* w, int64_t ldw, float* buf, int64_t ldb, float* alpha, int64_t lda,
                      const float* target, int64_t ldt, const float* theta, const int32_t* agents,
                      const int32_t* first, int32_t m, int64_t P, int32_t alg, float rho, float lr, float momentum,
                      int32_t local_steps, float* theta_out, float scale, double* resid_total, void* work,
                      hipStream_t s) {
  if (alg < DOL_FED_AVG || alg > DOL_FED_ADMM) return fail(DOL_EINVAL, "%s: algorithm must be 0 (FedAvg), 1 (FedProx) or 2 (FedADMM)", nm);
  const bool dual = alg == DOL_FED_ADMM;
  if (!dual) {
    if (alpha) return fail(DOL_EINVAL, "%s: FedAvg / FedProx have no duals (alpha must be NULL)", nm);
    lda = 0;
  }
  DOL_DIMS_OK(nm, ldw, ldb, lda, ldt, P);
  if (P < 0 || local_steps < 0) return fail(DOL_EINVAL, "%s: negative size", nm);
  if (!(scale > 0.0f)) return fail(DOL_EINVAL, "%s: scale must be > 0", nm);
  const bool mom = momentum != 0.0f;
  if (P > 0 && (!w || (dual && !alpha) || !target || !theta || !theta_out || (mom && !buf)))
    return fail(DOL_EINVAL, "%s: null pointer", nm);
  if (theta_out == w || (dual && theta_out == alpha) || theta_out == target || (mom && theta_out == buf))
    return fail(DOL_EINVAL, "%s: theta_out aliases the rows", nm);
  DOL_CHECKED(check_strip_round(nm, m, "the average indexes w[0]", P,
                                ldw < P || (dual && lda < P) || ldt < P || (mom && ldb < P), resid_total, work));
  if (P == 0) {
    if (resid_total) (void)hipMemsetAsync(resid_total, 0, 2 * sizeof(double), s);
    return check_launch(nm);
  }
  const int do_div = scale != 1.0f;
  launch_strips(P, {{w, ldw}, {alpha, lda}, {target, ldt}, {theta, 0}, {theta_out, 0}, {mom ? buf : nullptr, ldb}},
                resid_total, dual ? 2 : 1, work, s, [&](auto vt, const Strip& st) {
    dispatch([&](auto mc, auto rc, auto ntc, auto tc) {
      hipLaunchKernelGGL((admm_ls_round_mean_kernel<decltype(vt), decltype(mc)::value, decltype(rc)::value,
                                                    decltype(ntc)::value, decltype(tc)::value>),
                         dim3(static_cast<unsigned>(st.blocks)), dim3(st.nt), 0, s, w, ldw, buf, ldb, alpha, lda, target,
                         ldt, theta, agents, first, m, st.c_off, st.ncols, rho, -lr, momentum, local_steps, theta_out,
                         scale, do_div, st.partial, st.part_off, st.part_stride);
    }, Bool{mom}, Bool{resid_total != nullptr}, Ints<1024, 256>{st.nt}, Ints<0, 1, 2>{alg});
  });
  // FedAvg / FedProx: no ||alpha||^2 partials were written; the second total is 0
  if (resid_total && !dual) (void)hipMemsetAsync(resid_total + 1, 0, sizeof(double), s);
  return check_launch(nm);
}

}  // namespace

extern "C" {

int dol_prox_admm_sgd_f32(float* w, int64_t ldw, float* buf, int64_t ldb, float* g, int64_t ldg,
                          const float* theta, const float* alpha, int64_t lda, float rho, float lr,
                          float momentum, int first_step, int write_grad, int32_t n_agents,
                          int64_t P, hipStream_t s) {
  DOL_DIMS_OK("dol_prox_admm_sgd_f32", ldw, ldb, ldg, lda, P);
  DOL_CHECKED(check_size("dol_prox_admm_sgd_f32", n_agents < 0 || P < 0, n_agents == 0 || P == 0));
  if (!w || !g) return fail(DOL_EINVAL, "dol_prox_admm_sgd_f32: null w or g");
  if (alpha && !theta) return fail(DOL_EINVAL, "dol_prox_admm_sgd_f32: alpha without theta");
  const int mode = momentum_mode(momentum, first_step);
  if (mode != 0 && !buf) return fail(DOL_EINVAL, "dol_prox_admm_sgd_f32: momentum needs buf");
  if (ldw < P || ldg < P || (mode != 0 && ldb < P) || (alpha && lda < P))
    return fail(DOL_EINVAL, "dol_prox_admm_sgd_f32: ld < P");
  const bool vec_ok = row_vec_ok(w, ldw) && row_vec_ok(g, ldg) && (mode == 0 || row_vec_ok(buf, ldb)) &&
                      row_vec_ok(theta, 0) && row_vec_ok(alpha, alpha ? lda : 0);
  const ColSplit cs = split_cols(P, vec_ok);
  if (mul_sat(cdiv(cs.n4 + cs.tail, kThreads), n_agents) > kMaxBlocks)
    return fail(DOL_EINVAL, "dol_prox_admm_sgd_f32: problem too large for one launch");
  const int terms = (theta != nullptr) + (alpha != nullptr);  // 0 plain SGD, 1 prox (theta), 2 ADMM (theta and alpha)
  auto launch = [&](auto vtag, int64_t c_off, int64_t nc) {
    const int64_t nct = cdiv(nc, kThreads);
    dispatch([&](auto tc, auto mc, auto wg) {
      constexpr int T = decltype(tc)::value;
      // alpha is only read on this path (the kernel's pointer is non-const for the fused-dual variant)
      hipLaunchKernelGGL((prox_sgd_kernel<decltype(vtag), T >= 1, T == 2, decltype(mc)::value, decltype(wg)::value>),
                         dim3(static_cast<unsigned>(nct * n_agents)), dim3(kThreads), 0, s, w, ldw, buf, ldb, g, ldg,
                         theta, const_cast<float*>(alpha), lda, rho, -lr, momentum, c_off, nc, nct);
    }, Ints<0, 1, 2>{terms}, Ints<0, 1, 2>{mode}, Bool{write_grad != 0});
  };
  if (cs.n4 > 0) launch(f4{}, 0, cs.n4);
  if (cs.tail > 0) launch(float{}, cs.n4 * 4, cs.tail);
  return check_launch("dol_prox_admm_sgd_f32");
}

int dol_admm_step_dual_f32(float* w, int64_t ldw, float* buf, int64_t ldb, float* g, int64_t ldg,
                           const float* theta, float* alpha, int64_t lda, float rho, float lr,
                           float momentum, int first_step, int write_grad, int32_t n_agents, int64_t P,
                           hipStream_t s) {
  DOL_DIMS_OK("dol_admm_step_dual_f32", ldw, ldb, ldg, lda, P);
  DOL_CHECKED(check_rows("dol_admm_step_dual_f32", n_agents < 0 || P < 0, n_agents == 0 || P == 0,
                         !w || !g || !theta || !alpha, false, false));
  const int mode = momentum_mode(momentum, first_step);
  if (mode != 0 && !buf) return fail(DOL_EINVAL, "dol_admm_step_dual_f32: momentum needs buf");
  if (ldw < P || ldg < P || lda < P || (mode != 0 && ldb < P)) return fail(DOL_EINVAL, "dol_admm_step_dual_f32: ld < P");
  const bool vec_ok = row_vec_ok(w, ldw) && row_vec_ok(g, ldg) && (mode == 0 || row_vec_ok(buf, ldb)) &&
                      row_vec_ok(theta, 0) && row_vec_ok(alpha, lda);
  const ColSplit cs = split_cols(P, vec_ok);
  if (mul_sat(cdiv(cs.n4 + cs.tail, kThreads), n_agents) > kMaxBlocks) return fail(DOL_EINVAL, "dol_admm_step_dual_f32: too large");
  auto launch = [&](auto vtag, int64_t c_off, int64_t nc) {
    const int64_t nct = cdiv(nc, kThreads);
    dispatch([&](auto mc, auto wg) {
      hipLaunchKernelGGL((prox_sgd_kernel<decltype(vtag), true, true, decltype(mc)::value, decltype(wg)::value, true>),
                         dim3(static_cast<unsigned>(nct * n_agents)), dim3(kThreads), 0, s, w, ldw, buf, ldb, g, ldg,
                         theta, alpha, lda, rho, -lr, momentum, c_off, nc, nct);
    }, Ints<0, 1, 2>{mode}, Bool{write_grad != 0});
  };
  if (cs.n4 > 0) launch(f4{}, 0, cs.n4);
  if (cs.tail > 0) launch(float{}, cs.n4 * 4, cs.tail);
  return check_launch("dol_admm_step_dual_f32");
}

int dol_prox_grad_f32(float* g, int64_t ldg, const float* w, int64_t ldw, const float* theta,
                      const float* alpha, int64_t lda, float rho, int32_t n_agents, int64_t P,
                      hipStream_t s) {
  DOL_DIMS_OK("dol_prox_grad_f32", ldg, ldw, lda, P);
  DOL_CHECKED(check_rows("dol_prox_grad_f32", n_agents < 0 || P < 0, n_agents == 0 || P == 0, !g || !w || !theta,
                         ldg < P || ldw < P || (alpha && lda < P), false));
  const bool vec_ok = row_vec_ok(g, ldg) && row_vec_ok(w, ldw) && row_vec_ok(theta, 0) &&
                      row_vec_ok(alpha, alpha ? lda : 0);
  const ColSplit cs = split_cols(P, vec_ok);
  auto launch = [&](auto vtag, int64_t c_off, int64_t nc) {
    using V = decltype(vtag);
    const int64_t nct = cdiv(nc, kThreads);
    const dim3 grid(static_cast<unsigned>(nct * n_agents));
    dispatch([&](auto al) {
      hipLaunchKernelGGL((prox_grad_kernel<V, decltype(al)::value>), grid, dim3(kThreads), 0, s, g, ldg, w, ldw, theta,
                         alpha, lda, rho, c_off, nc, nct);
    }, Bool{alpha != nullptr});
  };
  if (mul_sat(cdiv(cs.n4 + cs.tail, kThreads), n_agents) > kMaxBlocks) return fail(DOL_EINVAL, "dol_prox_grad_f32: too large");
  if (cs.n4 > 0) launch(f4{}, 0, cs.n4);
  if (cs.tail > 0) launch(float{}, cs.n4 * 4, cs.tail);
  return check_launch("dol_prox_grad_f32");
}

int64_t dol_admm_dual_workspace_bytes(int32_t n_agents, int64_t P) {
  if (n_agents <= 0 || P <= 0 || P > dol::kMaxDim) return 0;
  // the scalar path has the most chunks: cdiv(P, kThreads*kDualIters)
  return int64_t(n_agents) * cdiv(P, int64_t(kThreads) * kDualIters) * int64_t(sizeof(double));
}

int dol_admm_dual_f32(float* alpha, int64_t lda, const float* w, int64_t ldw, const float* theta,
                      float rho, int32_t n_agents, int64_t P, double* resid_sq, void* work,
                      hipStream_t s) {
  DOL_DIMS_OK("dol_admm_dual_f32", lda, ldw, P);
  DOL_CHECKED(check_size("dol_admm_dual_f32", n_agents < 0 || P < 0, n_agents == 0));
  if (P > 0 && (!alpha || !w || !theta)) return fail(DOL_EINVAL, "dol_admm_dual_f32: null pointer");
  if (resid_sq && !work && P > 0) return fail(DOL_EINVAL, "dol_admm_dual_f32: resid_sq needs a workspace");
  if (lda < P || ldw < P) return fail(DOL_EINVAL, "dol_admm_dual_f32: ld < P");
  if (P == 0) {
    if (resid_sq) (void)hipMemsetAsync(resid_sq, 0, sizeof(double) * n_agents, s);
    return check_launch("dol_admm_dual_f32");
  }
  const bool vec = row_vec_ok(alpha, lda) && row_vec_ok(w, ldw) && row_vec_ok(theta, 0);
  const int64_t chunks = row_chunks(P, vec, n_agents);
  if (!chunks) return fail(DOL_EINVAL, "dol_admm_dual_f32: problem too large");
  double* partial = static_cast<double*>(work);
  const dim3 grid(static_cast<unsigned>(chunks * n_agents));
  dispatch([&](auto vc, auto rc) {
    hipLaunchKernelGGL((admm_dual_kernel<decltype(vc)::value, decltype(rc)::value>), grid, dim3(kThreads), 0, s, alpha,
                       lda, w, ldw, theta, rho, P, chunks, partial);
  }, Bool{vec}, Bool{resid_sq != nullptr});
  if (resid_sq) hipLaunchKernelGGL(resid_reduce_kernel, dim3(n_agents), dim3(kThreads), 0, s, partial, chunks, resid_sq);
  return check_launch("dol_admm_dual_f32");
}

int64_t dol_admm_ls_round_workspace_bytes(int32_t m, int64_t P) {
  if (m <= 0 || P <= 0 || P > dol::kMaxDim) return 0;
  return 2 * dol_admm_dual_workspace_bytes(m, P);  // ||w - theta||^2 and ||alpha||^2 partials
}

int dol_fed_ls_round_f32(float* w, int64_t ldw, float* buf, int64_t ldb, float* alpha, int64_t lda,
                         const float* target, int64_t ldt, const float* theta, const int32_t* agents,
                         const int32_t* first, int32_t m, int64_t P, int32_t algorithm, float rho, float lr,
                         float momentum, int32_t local_steps, double* resid_sq, double* alpha_sq, void* work,
                         hipStream_t s) {
  return fed_ls_round("dol_fed_ls_round_f32", w, ldw, buf, ldb, alpha, lda, target, ldt, theta, agents, first, m, P,
                      algorithm, rho, lr, momentum, local_steps, resid_sq, alpha_sq, work, s);
}

int dol_admm_ls_round_f32(float* w, int64_t ldw, float* buf, int64_t ldb, float* alpha, int64_t lda,
                          const float* target, int64_t ldt, const float* theta, const int32_t* agents,
                          const int32_t* first, int32_t m, int64_t P, float rho, float lr, float momentum,
                          int32_t local_steps, double* resid_sq, double* alpha_sq, void* work, hipStream_t s) {
  return fed_ls_round("dol_admm_ls_round_f32", w, ldw, buf, ldb, alpha, lda, target, ldt, theta, agents, first, m, P,
                      DOL_FED_ADMM, rho, lr, momentum, local_steps, resid_sq, alpha_sq, work, s);
}

int64_t dol_admm_ls_round_mean_workspace_bytes(int64_t P) {
  if (P <= 0 || P > dol::kMaxDim) return 0;
  return 2 * (cdiv(P, 64) + 2) * int64_t(sizeof(double));  // [2][blocks]: (w - theta)^2, alpha^2 (64-lane blocks)
}

int dol_fed_ls_round_mean_f32(float* w, int64_t ldw, float* buf, int64_t ldb, float* alpha, int64_t lda,
                              const float* target, int64_t ldt, const float* theta, const int32_t* agents,
                              const int32_t* first, int32_t m, int64_t P, int32_t algorithm, float rho, float lr,
                              float momentum, int32_t local_steps, float* theta_out, float scale,
                              double* resid_total, void* work, hipStream_t s) {
  return fed_ls_round_mean("dol_fed_ls_round_mean_f32", w, ldw, buf, ldb, alpha, lda, target, ldt, theta, agents,
                           first, m, P, algorithm, rho, lr, momentum, local_steps, theta_out, scale, resid_total,
                           work, s);
}

int dol_admm_ls_round_mean_f32(float* w, int64_t ldw, float* buf, int64_t ldb, float* alpha, int64_t lda,
                               const float* target, int64_t ldt, const float* theta, const int32_t* agents,
                               const int32_t* first, int32_t m, int64_t P, float rho, float lr, float momentum,
                               int32_t local_steps, float* theta_out, float scale, double* resid_total, void* work,
                               hipStream_t s) {
  return fed_ls_round_mean("dol_admm_ls_round_mean_f32", w, ldw, buf, ldb, alpha, lda, target, ldt, theta, agents,
                           first, m, P, DOL_FED_ADMM, rho, lr, momentum, local_steps, theta_out, scale, resid_total,
                           work, s);
}

int dol_scaffold_ls_round_f32(float* w, int64_t ldw, float* buf, int64_t ldb, float* ci, int64_t ldc,
                              const float* target, int64_t ldt, const float* theta, const float* c,
                              const int32_t* agents, const int32_t* first, int32_t m, int64_t P, float lr,
                              float momentum, int32_t local_steps, float inv_steps_lr, float global_lr,
                              float* theta_out, float scale_w, float* c_out, float scale_c, double* resid_total,
                              void* work, hipStream_t s) {
  const char* nm = "dol_scaffold_ls_round_f32";
  DOL_DIMS_OK(nm, ldw, ldb, ldc, ldt, P);
  if (P < 0) return fail(DOL_EINVAL, "%s: negative size", nm);
  if (local_steps < 1) return fail(DOL_EINVAL, "%s: local_steps must be >= 1", nm);
  if (!(scale_w > 0.0f) || !(scale_c > 0.0f)) return fail(DOL_EINVAL, "%s: scale_w and scale_c must be > 0", nm);
  const bool mom = momentum != 0.0f;
  if (P > 0 && (!w || !ci || !target || !theta || !c || !theta_out || !c_out || (mom && !buf)))
    return fail(DOL_EINVAL, "%s: null pointer", nm);
  for (const float* out : {static_cast<const float*>(theta_out), static_cast<const float*>(c_out)})
    if (out && (out == w || out == ci || out == target || (mom && out == buf)))
      return fail(DOL_EINVAL, "%s: %s aliases the rows", nm, out == theta_out ? "theta_out" : "c_out");
  if (theta_out && theta_out == c_out) return fail(DOL_EINVAL, "%s: theta_out and c_out alias", nm);
  DOL_CHECKED(check_strip_round(nm, m, "the chains start at the first sampled client", P,
                                ldw < P || ldc < P || ldt < P || (mom && ldb < P), resid_total, work));
  if (P == 0) {  // nothing to do but to zero the totals
    if (!resid_total) { g_err[0] = '\0'; return DOL_OK; }
    (void)hipMemsetAsync(resid_total, 0, 2 * sizeof(double), s);
    return check_launch(nm);
  }
  launch_strips(P, {{w, ldw}, {ci, ldc}, {target, ldt}, {theta, 0}, {c, 0}, {theta_out, 0}, {c_out, 0},
                    {mom ? buf : nullptr, ldb}},
                resid_total, 2, work, s, [&](auto vt, const Strip& st) {
    dispatch([&](auto mc, auto rc, auto ntc) {
      hipLaunchKernelGGL((scaffold_ls_round_kernel<decltype(vt), decltype(mc)::value, decltype(rc)::value,
                                                   decltype(ntc)::value>),
                         dim3(static_cast<unsigned>(st.blocks)), dim3(st.nt), 0, s, w, ldw, buf, ldb, ci, ldc, target, ldt,
                         theta, c, agents, first, m, st.c_off, st.ncols, -lr, momentum, local_steps, inv_steps_lr,
                         global_lr, theta_out, scale_w, c_out, scale_c, st.partial, st.part_off, st.part_stride);
    }, Bool{mom}, Bool{resid_total != nullptr}, Ints<1024, 256>{st.nt});
  });
  return check_launch(nm);
}

int dol_ordered_sum_f32(const float* W, int64_t ldw, const int32_t* order, int32_t m, int64_t P,
                        const float* acc_in, float* acc_out, float scale, hipStream_t s) {
  DOL_DIMS_OK("dol_ordered_sum_f32", ldw, P);
  DOL_CHECKED(check_size("dol_ordered_sum_f32", m < 0 || P < 0, P == 0));
  if (m == 0 && !acc_in) return fail(DOL_EINVAL, "dol_ordered_sum_f32: m == 0 needs acc_in");
  if (!acc_out || (m > 0 && (!W || !order))) return fail(DOL_EINVAL, "dol_ordered_sum_f32: null pointer");
  if (m > 0 && ldw < P) return fail(DOL_EINVAL, "dol_ordered_sum_f32: ld < P");
  if (!(scale > 0.0f)) return fail(DOL_EINVAL, "dol_ordered_sum_f32: scale must be > 0");
  const bool vec_ok = row_vec_ok(W, ldw) && row_vec_ok(acc_in, 0) && row_vec_ok(acc_out, 0);
  const ColSplit cs = split_cols(P, vec_ok);
  const int do_div = scale != 1.0f;
  if (cs.n4 > 0)
    hipLaunchKernelGGL(ordered_sum_kernel<f4>, dim3(static_cast<unsigned>(cdiv(cs.n4, kThreads))), dim3(kThreads), 0,
                       s, W, ldw, order, m, int64_t(0), cs.n4, acc_in, acc_out, scale, do_div);
  if (cs.tail > 0)
    hipLaunchKernelGGL(ordered_sum_kernel<float>, dim3(static_cast<unsigned>(cdiv(cs.tail, kThreads))), dim3(kThreads), 0,
                       s, W, ldw, order, m, cs.n4 * 4, cs.tail, acc_in, acc_out, scale, do_div);
  return check_launch("dol_ordered_sum_f32");
}

int dol_ordered_mean_f32(const float* W, int64_t ldw, const int32_t* order, int32_t m, int64_t P,
                         float* theta, hipStream_t s) {
  DOL_DIMS_OK("dol_ordered_mean_f32", ldw, P);
  if (m <= 0) return fail(DOL_EINVAL, "dol_ordered_mean_f32: m must be >= 1 (reference indexes w[0])");
  if (theta == W) return fail(DOL_EINVAL, "dol_ordered_mean_f32: theta aliases W");
  return dol_ordered_sum_f32(W, ldw, order, m, P, nullptr, theta, static_cast<float>(m), s);
}

}  // extern "C"
