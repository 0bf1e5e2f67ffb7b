// dol_launch.h — the host and device pieces that more than one translation
// unit of libdol_hip.so uses, each written once: launch arithmetic, the
// runtime-to-template dispatcher, the entry-point preamble, the f4 vector
// helpers and the mixing epilogues (the config-3 local step among them).
// Everything here has internal linkage (anonymous namespace), so the kernels
// instantiated over these types keep one definition per object.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

#include "../../include/dol_hip.h"
#include "dol_common.h"

// LDS-DMA operands (global_load_lds): the global source and the LDS destination
#define DOL_GPTR(p) ((const __attribute__((address_space(1))) void*)(p))
#define DOL_LPTR(p) ((__attribute__((address_space(3))) void*)(p))

namespace {
using dol::check_launch;
using dol::fail;
using dol::g_err;

// ----------------------------------------------------------------------------
// host-side launch helpers
// ----------------------------------------------------------------------------
constexpr int64_t kMaxBlocks = int64_t(1) << 24;

inline int64_t cdiv(int64_t a, int64_t b) { return a / b + (a % b != 0); }
// a * b saturated at INT64_MAX: block-count checks of absurd sizes must fail, not overflow
inline int64_t mul_sat(int64_t a, int64_t b) {
  int64_t r;
  return __builtin_mul_overflow(a, b, &r) ? INT64_MAX : r;
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
inline bool row_vec_ok(const void* base, int64_t ld) { return base == nullptr || (aligned16(base) && (ld % 4) == 0); }

// Split [0, P) into a f4 part and a scalar tail; vec_ok: whether the f4 path
// is legal for every (base, ld) pair of the call.
struct ColSplit {
  bool vec;
  int64_t n4;    // f4 columns
  int64_t tail;  // scalar columns after 4*n4 (or all P when !vec)
};
inline ColSplit split_cols(int64_t P, bool vec_ok) {
  if (!vec_ok) return {false, 0, P};
  return {true, P / 4, P % 4};
}

inline int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v && *v ? atoi(v) : dflt;
}

// compute units of the current device, asked once; 0 when there is none (each caller has its own fallback)
inline int n_cus() {
  static const int n = [] {
    int dev = 0, cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      cu = 0;
    return cu > 0 ? cu : 0;
  }();
  return n;
}

// SGD momentum mode of a step: 0 = none, 1 = first step (buf = g), 2 = buf = buf*mom + g
inline int momentum_mode(float momentum, int first_step) { return (momentum == 0.0f) ? 0 : (first_step ? 1 : 2); }

// Runtime values to template arguments: dispatch(f, Bool{b}, Ints<0, 1, 2>{m})
// calls the generic lambda f(std::bool_constant<b>{}, std::integral_constant<int, m>{}),
// one selector per argument, in order.  An int outside its list takes the last value.
struct Bool { bool v; };
template <int... Vs> struct Ints { int v; };

template <class F> auto dispatch(F&& f) { return f(); }
template <class F, class... R> auto dispatch(F&& f, Bool b, R... r);
template <class F, int V, int... Vs, class... R> auto dispatch(F&& f, Ints<V, Vs...> i, R... r);
template <class F, class K, class... R> auto dispatch_rest(F& f, K k, R... r) {
  return dispatch([&](auto... c) { return f(k, c...); }, r...);
}
template <class F, class... R> auto dispatch(F&& f, Bool b, R... r) {
  return b.v ? dispatch_rest(f, std::true_type{}, r...) : dispatch_rest(f, std::false_type{}, r...);
}
template <class F, int V, int... Vs, class... R> auto dispatch(F&& f, Ints<V, Vs...> i, R... r) {
  if constexpr (sizeof...(Vs) == 0) return dispatch_rest(f, std::integral_constant<int, V>{}, r...);
  else return i.v == V ? dispatch_rest(f, std::integral_constant<int, V>{}, r...) : dispatch(f, Ints<Vs...>{i.v}, r...);
}

// The opening checks of an entry point, in the order they all use: negative
// size, nothing to do, null pointer, short leading dimension, aliased output.
// Returns DOL_OK to go on, kEmpty for an empty problem (the caller returns
// DOL_OK; the message is cleared), else the refusal.  The two texts that
// differ between entry points are parameters.
constexpr int kEmpty = 1;
inline int check_size(const char* nm, bool negative, bool empty) {
  if (negative) return fail(DOL_EINVAL, "%s: negative size", nm);
  if (empty) { g_err[0] = '\0'; return kEmpty; }
  return DOL_OK;
}
inline int check_rows(const char* nm, bool negative, bool empty, bool null, bool ld_short, bool alias,
                      const char* alias_msg = "X and Y alias", const char* ld_msg = "ld < P") {
  if (const int rc = check_size(nm, negative, empty)) return rc;
  if (null) return fail(DOL_EINVAL, "%s: null pointer", nm);
  if (ld_short) return fail(DOL_EINVAL, "%s: %s", nm, ld_msg);
  if (alias) return fail(DOL_EINVAL, "%s: %s", nm, alias_msg);
  return DOL_OK;
}
#define DOL_CHECKED(call)                                                  \
  do {                                                                     \
    if (const int dol_rc_ = (call)) return dol_rc_ == kEmpty ? DOL_OK : dol_rc_; \
  } while (0)
constexpr const char* kJacobiAlias = "X and Y alias (Jacobi mix needs two buffers)";

// The five row matrices of a gradient-tracking round on an agent-major bank
// (X, S in; XO, SO out; the targets T) and the argument rules that
// dol_gt_ring_f32 and dol_gt_csr_f32 share, each written once.  An entry point
// calls check(), then its own rules (the ring's halos), then objective_ok(),
// and hands vec_ok() to split_cols.  (dol_gt_csr_pm_f32 validates for itself:
// gt_csr_pm_impl in pmajor.hip has other rules, in another order.)
struct GtRows {
  const float* X; int64_t ldx;
  const float* S; int64_t lds;
  float* XO; int64_t ldxo;
  float* SO; int64_t ldso;
  const float* T; int64_t ldt;

  // n rows of P columns; other_null: one of the entry point's own required pointers is null
  int check(const char* nm, int32_t n, int64_t P, bool other_null) const {
    DOL_DIMS_OK(nm, ldx, lds, ldxo, ldso, ldt, P);
    const bool alias = X == S || X == XO || X == SO || S == XO || S == SO || XO == SO;
    return check_rows(nm, n < 0 || P < 0, n == 0 || P == 0, !X || !S || !XO || !SO || !T || other_null,
                      ldx < P || lds < P || ldxo < P || ldso < P || ldt < P, alias,
                      "X, S, XO, SO alias (the Jacobi update of x and s needs four buffers)");
  }
  static int objective_ok(const char* nm, int32_t objective) {
    return objective != 0 && objective != 1 ? fail(DOL_EINVAL, "%s: objective must be 0 or 1", nm) : DOL_OK;
  }
  bool vec_ok() const {
    return row_vec_ok(X, ldx) && row_vec_ok(S, lds) && row_vec_ok(XO, ldxo) && row_vec_ok(SO, ldso) &&
           row_vec_ok(T, ldt);
  }
};

// ----------------------------------------------------------------------------
// vector helpers: the same kernel body runs on float (tail / unaligned) and
// f4 (main stream).  All arithmetic is explicit per lane so that each
// product and sum rounds once, exactly as the reference's torch CPU ops.
// ----------------------------------------------------------------------------
typedef float f4 __attribute__((ext_vector_type(4)));  // native 16-B vector (nontemporal builtins need it)
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr uint32_t kOOB = 0x80000000u;  // a buffer offset past every range: the access is dropped

template <typename V> struct Vec;
template <> struct Vec<float> {
  static constexpr int W = 1;
};
template <> struct Vec<f4> {
  static constexpr int W = 4;
};

__device__ __forceinline__ float axpy0(float wp, float a, float wn, float b) {
  // ((+0 + wp*a) + wn*b) with every operation rounded (no contraction)
  float acc = 0.0f;
  acc = acc + wp * a;
  acc = acc + wn * b;
  return acc;
}
__device__ __forceinline__ f4 axpy0(float wp, f4 a, float wn, f4 b) {
  return f4{axpy0(wp, a.x, wn, b.x), axpy0(wp, a.y, wn, b.y),
            axpy0(wp, a.z, wn, b.z), axpy0(wp, a.w, wn, b.w)};
}
// (ring_steps_kernel with 8-B lanes and R = 22-54: 11.25-11.65 ms vs 11.24-11.27
// for f4 / R = 22 at eps = 5, 8192 x 2^20, same box: kept f4)
__device__ __forceinline__ float fmac(float acc, float a, float x) { return acc + a * x; }
__device__ __forceinline__ f4 fmac(f4 acc, float a, f4 x) {
  return f4{acc.x + a * x.x, acc.y + a * x.y, acc.z + a * x.z, acc.w + a * x.w};
}
__device__ __forceinline__ float vzero(float) { return 0.0f; }
__device__ __forceinline__ f4 vzero(f4) { return f4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ float vadd(float a, float b) { return a + b; }
__device__ __forceinline__ f4 vadd(f4 a, f4 b) {
  return f4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
}
__device__ __forceinline__ float vdiv(float a, float s) { return a / s; }
__device__ __forceinline__ f4 vdiv(f4 a, float s) {
  return f4{a.x / s, a.y / s, a.z / s, a.w / s};
}

template <typename V, bool NT>
__device__ __forceinline__ V ldv(const V* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <typename V, bool NT>
__device__ __forceinline__ void stv(V* p, V v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// ----------------------------------------------------------------------------
// Mixing epilogues.  NoEpi: Y = W X (the gossip round).  DgdEpi: then `steps`
// local momentum-SGD iterations per agent on a separable synthetic loss —
// BASELINE config 3, decentralised gradient descent in the reference's round
// order (DIST/simulators.py:147-162: consensus, then local_update with the
// optimizer of DIST/clients.py:43-49) — so a round streams X, the targets and
// the momentum once.  Rounding as oracle_dgd_local_f32:
//   OBJ 0 least squares  g = x - t;   OBJ 1 logistic  g = -t / (1 + exp(t x))
//   MODE 0 plain SGD; 1 momentum, first step (buf = g); 2 momentum (buf = buf*mom + g)
//   x = fma(-lr, d, x)
// load() is issued with the mixing loads; apply() runs after the mix.
// ----------------------------------------------------------------------------
// The gradient of the separable loss on one coordinate, written once: the local
// steps below, the gradient-tracking round (csr_pm_gt_kernel) and
// dol_separable_grad_f32 all call it.
template <int OBJ>
__device__ __forceinline__ float separable_grad(float x, float t) {
  if constexpr (OBJ == 0) return x - t;
  else return -t / (1.0f + expf(t * x));
}

// The gradient-tracking round (DIGing / NEXT) on one coordinate after its two
// mixes ax = (W_off x), as = (W_off s): the one place this arithmetic is written
// (csr_pm_gt_kernel, gt_ring_*_kernel, gt_csr_*_kernel), which is why the three
// rounds agree bit for bit whenever their mixes do.  All fp32, each operation
// rounded once (-ffp-contract=off), d the agent's self weight:
//   self:  ax = fl(ax + fl(d x));  as = fl(as + fl(d s))
//   x' = fma(-lr, s, ax)
//   s' = fl(fl(as + g(x', t)) - g(x, t))                     g = separable_grad<OBJ>
// self is a compile-time constant on the agent-major banks and the kernel's
// run-time "self weights given" on the parameter-major one.
template <int OBJ>
__device__ __forceinline__ void gt_finish(float ax, float as, float x, float s, float t, float d, bool self,
                                          float neg_lr, float& xo, float& so) {
  if (self) {
    ax = ax + d * x;
    as = as + d * s;
  }
  xo = __builtin_fmaf(neg_lr, s, ax);
  so = (as + separable_grad<OBJ>(xo, t)) - separable_grad<OBJ>(x, t);
}
// the same on four coordinates; d: one agent's weight (agent-major) or four agents' (parameter-major)
template <int OBJ, class D>
__device__ __forceinline__ void gt_finish(f4 ax, f4 as, f4 x, f4 s, f4 t, D d, bool self, float neg_lr, f4& xo,
                                          f4& so) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float dj, xe, se;
    if constexpr (std::is_same_v<D, f4>) dj = d[j];
    else dj = d;
    gt_finish<OBJ>(ax[j], as[j], x[j], s[j], t[j], dj, self, neg_lr, xe, se);
    xo[j] = xe;
    so[j] = se;
  }
}

// The push-sum gradient-tracking round (ADD-OPT / Push-DIGing) on one coordinate
// after its two mixes au = (C_off u), as = (C_off s), written once
// (gt_push_csr_*_kernel): gt_finish with the gradient taken at the de-biased
// estimate z = u / v instead of at u.  v: the agent's push-sum weight before
// the round, av: after it (C v, self term included; the caller computes it
// once per agent).  All fp32, each operation rounded once, the divisions
// correctly rounded (a zero v divides like IEEE):
//   self:  au = fl(au + fl(d u));  as = fl(as + fl(d s))
//   u' = fma(-lr, s, au)
//   z = u / v;  z' = u' / av
//   s' = fl(fl(as + g(z', t)) - g(z, t))                     g = separable_grad<OBJ>
template <int OBJ>
__device__ __forceinline__ void gt_push_finish(float au, float as, float u, float s, float t, float d, bool self,
                                               float neg_lr, float v, float av, float& uo, float& so) {
  if (self) {
    au = au + d * u;
    as = as + d * s;
  }
  uo = __builtin_fmaf(neg_lr, s, au);
  const float z = __fdiv_rn(u, v);
  const float zo = __fdiv_rn(uo, av);
  so = (as + separable_grad<OBJ>(zo, t)) - separable_grad<OBJ>(z, t);
}
// the same on four coordinates of one agent
template <int OBJ>
__device__ __forceinline__ void gt_push_finish(f4 au, f4 as, f4 u, f4 s, f4 t, float d, bool self, float neg_lr,
                                               float v, float av, f4& uo, f4& so) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float ue, se;
    gt_push_finish<OBJ>(au[j], as[j], u[j], s[j], t[j], d, self, neg_lr, v, av, ue, se);
    uo[j] = ue;
    so[j] = se;
  }
}

// The gradient-FED gradient-tracking round on one coordinate after its two
// mixes (gt_grad_csr_*_kernel, grad_rounds.hip): DIGing with the tracker update
// at the front of the round, s_k = W s_{k-1} + G_k - G_{k-1}, then x_{k+1} = W
// x_k - lr s_k, the gradients g (this round's) and gp (last round's) read from
// rows that something else computed.  All fp32, each operation rounded once, d
// the agent's self weight:
//   self:  ax = fl(ax + fl(d x));  as = fl(as + fl(d s))
//   s' = fl(fl(as + g) - gp)
//   x' = fma(-lr, s', ax)
// x' takes the agent's own new tracker, so the round is one pass; from s = 0 and
// gp = 0 the first round gives s' = g.  Without self weights x and s are not read.
__device__ __forceinline__ void gt_grad_finish(float ax, float as, float x, float s, float g, float gp, float d,
                                               bool self, float neg_lr, float& xo, float& so) {
  if (self) {
    ax = ax + d * x;
    as = as + d * s;
  }
  so = (as + g) - gp;
  xo = __builtin_fmaf(neg_lr, so, ax);
}
// the same on four coordinates of one agent
__device__ __forceinline__ void gt_grad_finish(f4 ax, f4 as, f4 x, f4 s, f4 g, f4 gp, float d, bool self, float neg_lr,
                                               f4& xo, f4& so) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float xe, se;
    gt_grad_finish(ax[j], as[j], x[j], s[j], g[j], gp[j], d, self, neg_lr, xe, se);
    xo[j] = xe;
    so[j] = se;
  }
}

// The EXTRA round (Shi, Ling, Wu, Yin, SIAM J. Optim. 25(2), 2015) on one
// coordinate after its one mix ax = (W_off x), written once (ExtraEpi below, so
// every agent-major mix kernel that takes an epilogue, and csr_pm_extra_kernel
// on the parameter-major bank).  With W~ = (I + W) / 2
// the method's two-step recursion is x' = W x - lr g(x) - c, c' = c + (x - W x) / 2,
// c(0) = 0: the correction c is the agent's own row, so only x is mixed.  All
// fp32, each operation rounded once, d the agent's self weight:
//   self:  ax = fl(ax + fl(d x))
//   r  = fl(x - ax)
//   x' = fl(fma(-lr, g(x, t), ax) - c)                       g = separable_grad<OBJ>
//   c' = fma(0.5, r, c)
// OBJ == kObjGradRow is the gradient-FED round (dol_extra_grad_csr_f32 only):
// the row loaded in the target's place IS the gradient, g = t, and
// separable_grad is not called.
constexpr int kObjGradRow = 2;
template <int OBJ>
__device__ __forceinline__ void extra_finish(float ax, float x, float c, float t, float d, bool self, float neg_lr,
                                             float& xo, float& co) {
  if (self) ax = ax + d * x;
  const float r = x - ax;
  float g;
  if constexpr (OBJ == kObjGradRow) g = t;
  else g = separable_grad<OBJ>(x, t);
  xo = __builtin_fmaf(neg_lr, g, ax) - c;
  co = __builtin_fmaf(0.5f, r, c);
}
// the same on four coordinates; d: one agent's weight (agent-major) or four agents' (parameter-major)
template <int OBJ, class D>
__device__ __forceinline__ void extra_finish(f4 ax, f4 x, f4 c, f4 t, D d, bool self, float neg_lr, f4& xo,
                                             f4& co) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float dj, xe, ce;
    if constexpr (std::is_same_v<D, f4>) dj = d[j];
    else dj = d;
    extra_finish<OBJ>(ax[j], x[j], c[j], t[j], dj, self, neg_lr, xe, ce);
    xo[j] = xe;
    co[j] = ce;
  }
}

// The local steps on one coordinate: the one place this arithmetic is written
// (DgdEpi on the agent-major bank, csr_pm_kernel on the parameter-major one).
// e: the epilogue's arguments, read where they are used (e.steps, e.mom, e.neg_lr).
template <int OBJ, int MODE, class E>
__device__ __forceinline__ float dgd_local_steps(float x, float t, float& b, const E& e) {
  for (int s = 0; s < e.steps; ++s) {
    const float g = separable_grad<OBJ>(x, t);
    float d = g;
    if constexpr (MODE != 0) {
      if (MODE == 1 && s == 0) b = g;
      else b = b * e.mom + g;
      d = b;
    }
    x = __builtin_fmaf(e.neg_lr, d, x);
  }
  return x;
}

// An epilogue whose kCentre is true takes the mixed row's own value from a
// kernel that holds it in registers (the ring kernels' stencil window) through
// apply_centre(y, centre, state, r, cf); the others, and every kernel without
// such a window, use apply().  The kernels branch on it with `if constexpr`,
// their apply() call left as it was.
struct Empty {};
struct NoEpi {
  static constexpr bool kCentre = false;
  template <typename V> __device__ __forceinline__ Empty load(int, int64_t) const { return {}; }
  template <typename V> __device__ __forceinline__ V apply(V y, Empty, int, int64_t) const { return y; }
};

// One read-once element of an epilogue's own row (targets, momentum,
// corrections) under the policy DgdEpi's comment below measures: nt 3 = buffer
// load with aux 3 (sc0 nt), 1 = the compiler's nontemporal global load, 0 =
// plain.  Scalar columns always load plainly.
template <typename V>
__device__ __forceinline__ V epi_ld(int nt, const float* row, int64_t cf) {
  const V* p = reinterpret_cast<const V*>(row + cf);
  if constexpr (sizeof(V) == 16) {
    if (nt == 3) {
      const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, 0x7ffffff0, 0x00020000);
      return __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(rs, uint32_t(cf) * 4u, 0, 3));
    }
    if (nt == 1) return __builtin_nontemporal_load(p);
  }
  return *p;
}
// DOL_DGD_EPI_NT (default 3) for rows of P floats: buffer offsets are 32-bit
// (rows of < 2^29 floats); longer rows take plain loads
inline int epi_nt_policy(int64_t P) {
  static const int nt_env = env_int("DOL_DGD_EPI_NT", 3);
  return (nt_env == 3 && P > (int64_t(1) << 29) - 16) ? 0 : nt_env;
}

template <typename V> struct DgdState { V t, b; };

template <int OBJ, int MODE>
struct DgdEpi {
  static constexpr bool kCentre = false;
  const float* __restrict__ T; int64_t ldt;
  float* __restrict__ M; int64_t ldm;
  float neg_lr, mom;
  int steps;
  // Target / momentum rows are read once: buffer loads with the nontemporal
  // policy (aux 3 = sc0 nt), so they do not push the X halo rows -- re-read by
  // the next row group's tile, 1024 workgroups later -- out of the XCD's L2.
  // With plain loads the ring round read 1.16x its bytes (14.97 vs 12.88 GB
  // at 1024 x 2^20, least squares + momentum) and ran 3.58-3.59 ms; with these
  // 12.90 GB = 1.00x and 3.44-3.45 ms (profiles/r06f_dgd_epi_policy.jsonl; sc0
  // sc1 without nt: no change).  DOL_DGD_EPI_NT=0 restores plain loads, 1 the
  // compiler's nontemporal global loads (the switch stays: it is this runtime
  // branch, inside every DGD kernel).
  int nt;

  template <typename V> __device__ __forceinline__ V ld(const float* row, int64_t cf) const {
    return epi_ld<V>(nt, row, cf);
  }
  template <typename V> __device__ __forceinline__ DgdState<V> load(int r, int64_t cf) const {
    DgdState<V> st;
    st.t = ld<V>(T + int64_t(r) * ldt, cf);
    if constexpr (MODE == 2) st.b = ld<V>(M + int64_t(r) * ldm, cf);
    else st.b = vzero(V{});
    return st;
  }
  template <typename V> __device__ __forceinline__ V apply(V y, DgdState<V> st, int r, int64_t cf) const {
    if constexpr (Vec<V>::W == 1) {
      y = dgd_local_steps<OBJ, MODE>(y, st.t, st.b, *this);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float bj = st.b[j];
        y[j] = dgd_local_steps<OBJ, MODE>(y[j], st.t[j], bj, *this);
        st.b[j] = bj;
      }
    }
    if constexpr (MODE != 0) __builtin_nontemporal_store(st.b, reinterpret_cast<V*>(M + int64_t(r) * ldm + cf));
    return y;
  }
};

// validation + dispatch of the BASELINE config-3 round (mix + local steps)
struct DgdArgs {
  const float* T; int64_t ldt; float* M; int64_t ldm;
  int32_t objective, steps; float lr, momentum; int first_step;
};

inline int check_dgd(const char* nm, const DgdArgs& d, int64_t P, bool* evec, int* mode) {
  if (!d.T) return fail(DOL_EINVAL, "%s: null target", nm);
  if (d.objective != 0 && d.objective != 1) return fail(DOL_EINVAL, "%s: objective must be 0 (least squares) or 1 (logistic)", nm);
  if (d.steps < 1) return fail(DOL_EINVAL, "%s: local_steps must be >= 1", nm);
  if (d.ldt < P) return fail(DOL_EINVAL, "%s: ldt < P", nm);
  *mode = momentum_mode(d.momentum, d.first_step);
  if (*mode != 0 && (!d.M || d.ldm < P)) return fail(DOL_EINVAL, "%s: momentum needs a momentum buffer with ldm >= P", nm);
  *evec = row_vec_ok(d.T, d.ldt) && (*mode == 0 || row_vec_ok(d.M, d.ldm));
  return DOL_OK;
}

// Checks d (unless the problem is empty: the mix's own preamble then answers)
// and calls f(epi, epi_vec_ok) with the epilogue of d's objective and mode.
template <class F>
int with_dgd_epi(const char* nm, const DgdArgs& d, bool empty, int64_t P, F&& f) {
  bool evec = false;
  int mode = 0;
  if (!empty) {
    const int rc = check_dgd(nm, d, P, &evec, &mode);
    if (rc) return rc;
  }
  const int nt = epi_nt_policy(P);
  return dispatch([&](auto obj, auto md) {
    return f(DgdEpi<decltype(obj)::value, decltype(md)::value>{d.T, d.ldt, d.M, d.ldm, -d.lr, d.momentum, d.steps, nt}, evec);
  }, Ints<0, 1>{d.objective}, Ints<0, 1, 2>{mode});
}

// ExtraEpi: the EXTRA round (extra_finish above) as a mixing epilogue.  After
// the mix of row r it needs that row's own x, its correction c (read and
// written in place, like DgdEpi's M) and its target t.  t and c are read once:
// DgdEpi's nontemporal policy (epi_ld).  The centre x: CENTRE = false loads it
// in load() with the default policy (it is another row's neighbour) -- the CSR
// kernels and the ring's edge kernel, which do not hold it; CENTRE = true takes
// it from the kernel's stencil window through apply_centre (ring_mix_dma_kernel,
// ring_mix_kernel), which saves the second read of the row and a third of the
// epilogue's registers.
template <typename V> struct ExtraState { V t, c, x; };

template <int OBJ, bool SELF, bool CENTRE>
struct ExtraEpi {
  static constexpr bool kCentre = CENTRE;
  const float* __restrict__ T; int64_t ldt;
  float* __restrict__ C; int64_t ldc;
  const float* __restrict__ X; int64_t ldx;
  const float* __restrict__ self_w;
  float neg_lr;
  int nt;

  template <typename V> __device__ __forceinline__ ExtraState<V> load(int r, int64_t cf) const {
    ExtraState<V> st;
    st.t = epi_ld<V>(nt, T + int64_t(r) * ldt, cf);
    st.c = epi_ld<V>(nt, C + int64_t(r) * ldc, cf);
    if constexpr (CENTRE) st.x = vzero(V{});
    else st.x = *reinterpret_cast<const V*>(X + int64_t(r) * ldx + cf);
    return st;
  }
  template <typename V>
  __device__ __forceinline__ V apply_centre(V y, V centre, ExtraState<V> st, int r, int64_t cf) const {
    st.x = centre;
    return apply(y, st, r, cf);
  }
  template <typename V> __device__ __forceinline__ V apply(V y, ExtraState<V> st, int r, int64_t cf) const {
    float d = 0.0f;
    if constexpr (SELF) d = self_w[r];
    V xo, co;
    extra_finish<OBJ>(y, st.x, st.c, st.t, d, SELF, neg_lr, xo, co);
    __builtin_nontemporal_store(co, reinterpret_cast<V*>(C + int64_t(r) * ldc + cf));
    return xo;
  }
};

// validation + dispatch of the EXTRA round (mix + extra_finish)
struct ExtraArgs {
  const float* T; int64_t ldt; float* C; int64_t ldc; const float* self_w;
  int32_t objective; float lr;
};

// X, Y: the mix's own pair (the mix's preamble checks them; here only against
// corr).  fed: the gradient-fed round, whose T is the gradient matrix G (its
// name in the messages; no objective; G must not be the output Y either).
inline int check_extra(const char* nm, const ExtraArgs& e, const float* X, const float* Y, int64_t P, bool* evec,
                       bool fed = false) {
  if (!e.T) return fail(DOL_EINVAL, "%s: null %s", nm, fed ? "G" : "target");
  if (!e.C) return fail(DOL_EINVAL, "%s: null corr", nm);
  if (!fed && e.objective != 0 && e.objective != 1)
    return fail(DOL_EINVAL, "%s: objective must be 0 (least squares) or 1 (logistic)", nm);
  if (e.ldt < P) return fail(DOL_EINVAL, "%s: %s < P", nm, fed ? "ldg" : "ldt");
  if (e.ldc < P) return fail(DOL_EINVAL, "%s: ldc < P", nm);
  if (e.C == X || e.C == Y || e.C == e.T)
    return fail(DOL_EINVAL, "%s: corr aliases X, Y or %s (the correction is updated in place)", nm,
                fed ? "G" : "target");
  if (fed && e.T == Y) return fail(DOL_EINVAL, "%s: G aliases Y (the gradient rows are read while Y is written)", nm);
  *evec = row_vec_ok(e.T, e.ldt) && row_vec_ok(e.C, e.ldc);
  return DOL_OK;
}

// Checks e (unless the problem is empty: the mix's own preamble then answers)
// and calls f(epi, epi_vec_ok) with the epilogue of e's objective and of
// whether self weights are given; X / ldx: the rows the mix reads, whose row r
// is the centre of output row r.  CENTRE: whether the kernels f launches hand
// that row to the epilogue themselves (ExtraEpi).
template <bool CENTRE, class F>
int with_extra_epi(const char* nm, const ExtraArgs& e, const float* X, int64_t ldx, const float* Y, bool empty,
                   int64_t P, F&& f) {
  bool evec = false;
  if (!empty) {
    const int rc = check_extra(nm, e, X, Y, P, &evec);
    if (rc) return rc;
  }
  const int nt = epi_nt_policy(P);
  return dispatch([&](auto obj, auto self) {
    return f(ExtraEpi<decltype(obj)::value, decltype(self)::value, CENTRE>{e.T, e.ldt, e.C, e.ldc, X, ldx, e.self_w, -e.lr, nt},
             evec);
  }, Ints<0, 1>{e.objective}, Bool{e.self_w != nullptr});
}

// The same for the gradient-fed round: e.T is the gradient matrix G, e.objective
// is not read, and the epilogue is ExtraEpi<kObjGradRow, ...>, which no other
// path instantiates.
template <bool CENTRE, class F>
int with_extra_grad_epi(const char* nm, const ExtraArgs& e, const float* X, int64_t ldx, const float* Y, bool empty,
                        int64_t P, F&& f) {
  bool evec = false;
  if (!empty) {
    const int rc = check_extra(nm, e, X, Y, P, &evec, true);
    if (rc) return rc;
  }
  const int nt = epi_nt_policy(P);
  return dispatch([&](auto self) {
    return f(ExtraEpi<kObjGradRow, decltype(self)::value, CENTRE>{e.T, e.ldt, e.C, e.ldc, X, ldx, e.self_w, -e.lr, nt},
             evec);
  }, Bool{e.self_w != nullptr});
}

}  // namespace
