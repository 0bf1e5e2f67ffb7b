// gt_push_csr.hip — one push-sum gradient-tracking round (ADD-OPT, Xi-Xin-Khan
// 2018; Push-DIGing in combine-then-adapt form) on the agent-major bank with
// any sparse column-stochastic C in one HBM pass: dol_gt_push_csr_f32, the
// sibling of dol_gt_csr_f32 (gt_csr.hip) for weights that are not doubly
// stochastic.  Its own translation unit, so gt_csr.o and every pinned kernel
// stay as they are.
//
// Layout and mixes as gt_csr.hip: U (the push-sum numerators) and S (the
// trackers) are gathered through ONE read of rowptr / col / val per row; the
// centre rows u_i, s_i and the target row t_i ride along.  C = C_off +
// diag(self_w), C_off the CSR whose row i lists i's in-neighbours.  For every
// row i and column c, all fp32, each operation rounded once
// (-ffp-contract=off):
//   au = sum_e val[e] * u[col[e]]      (+0 start, ascending e: fmac())     as = the same over s
//   av = sum_e val[e] * v[col[e]]      (the same rounding, on the n-vector v)
//   av = fl(av + fl(d_i v_i)) with self weights;   v'_i = av
// and then gt_push_finish (dol_launch.h) with d = self_w[i], v = v[i], av =
// v'[i]: the gradients are taken at z = u / v and z' = u' / av, two correctly
// rounded divisions per coordinate.  z is not stored (it is U / v), so the
// round moves the five streams of dol_gt_csr_f32 plus 2 n floats.
//
// How v' is produced: gt_push_v_kernel (n threads) runs first in the same call
// and writes v_out; the main kernels, ordered after it on the stream, read
// v[i] and v_out[i] as two per-row scalars.  The degree-4 fast path's register
// budget is the reason: the mix of v inside the main kernels would add a third
// gather to it.
//
// Kernels: gt_csr_kernel's and gt_csr_xcd_kernel's geometry, policies and
// clamped ragged rows taken over unchanged (gt_csr.hip's header has the
// measurements: 512-B XCD-pinned tiles from 512 rows, 16 rows per block, the
// gathered and centre rows with the default policy, the target row nontemporal,
// nontemporal stores); none of that was measured again here.
//
// Resource usage, from the compiler's kernel-resource-usage remarks (gfx950,
// -O3; occupancy in waves per SIMD; no instantiation uses scratch or LDS):
//   kernel                           VGPRs: LS / LS+self / logistic / logistic+self   scratch   occupancy
//   gt_push_csr_xcd_kernel<32, 2>    118 / 119 / 126 / 122                            0         4
//   gt_push_csr_kernel<f4>           78 / 78 / 80 / 80                                0         6
//   gt_push_csr_kernel<float>        40 / 40 / 40 / 40                                0         8
//   gt_push_v_kernel                 12 (with and without self weights)               0         8
// The pinned kernel keeps gt_csr_xcd_kernel's 4 waves per SIMD (128 VGPRs): the
// two per-row scalars and the divisions' temporaries fit beside its 112-122.
#include "dol_launch.h"

namespace {
constexpr int kThreads = 256;  // 4 waves of 64
constexpr int kGtPushRows = 16;  // rows per block of gt_push_csr_kernel (gt_csr.hip's kGtCsrRows)
constexpr int kGtPushMinXcdRows = 512;  // the XCD-pinned form from this many rows (gt_csr.hip's rule)

struct GtPush {
  const float* U; int64_t ldu;
  const float* S; int64_t lds;
  float* UO; int64_t lduo;
  float* SO; int64_t ldso;
  const float* T; int64_t ldt;
  float neg_lr;
};
// (rowptr, col, val, the self weights and the two push-sum weight vectors are
// kernel arguments of their own, const __restrict__, as in gt_csr.hip)

// ----------------------------------------------------------------------------
// v' = C v, one thread per agent: the mix's rounding on a vector.
// ----------------------------------------------------------------------------
template <bool SELF>
__global__ __launch_bounds__(kThreads) void gt_push_v_kernel(int n_rows, const int32_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ col,
                                                             const float* __restrict__ val,
                                                             const float* __restrict__ wself,
                                                             const float* __restrict__ v, float* __restrict__ vout) {
  const int64_t r = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (r >= n_rows) return;
  const int e1 = rowptr[r + 1];
  float av = 0.0f;
  for (int e = rowptr[r]; e < e1; ++e) av = fmac(av, val[e], v[col[e]]);
  if (SELF) av = av + wself[r] * v[r];
  vout[r] = av;
}

// ----------------------------------------------------------------------------
// gt_csr_kernel's form: 4 KiB column tiles (V = f4) or 1 KiB of scalar columns
// (V = float: the P % 4 tail, or every column when a row base is not 16-B
// aligned), kGtPushRows rows per block, row group fastest: small graphs, and
// the f4 columns the pinned tiles leave over.  c_off: the first element column
// of this launch.
// ----------------------------------------------------------------------------
template <typename V, int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_push_csr_kernel(GtPush a, int n_rows, int64_t c_off, int64_t ncols_v,
                                                               int64_t n_row_groups,
                                                               const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col,
                                                               const float* __restrict__ val,
                                                               const float* __restrict__ wself,
                                                               const float* __restrict__ v,
                                                               const float* __restrict__ vnew) {
  constexpr int VW = Vec<V>::W;
  const int64_t b = blockIdx.x;
  const int rg = static_cast<int>(b % n_row_groups);
  const int64_t c = (b / n_row_groups) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  const int r0 = rg * kGtPushRows;
  const int r1 = min(r0 + kGtPushRows, n_rows);
  const int64_t cf = c_off + c * VW;  // element column
  const float* ub = a.U + cf;
  const float* sb = a.S + cf;
  auto uat = [&](int64_t r) { return *reinterpret_cast<const V*>(ub + r * a.ldu); };
  auto sat = [&](int64_t r) { return *reinterpret_cast<const V*>(sb + r * a.lds); };
  for (int r = r0; r < r1; ++r) {
    const V t = ldv<V, sizeof(V) == 16>(reinterpret_cast<const V*>(a.T + int64_t(r) * a.ldt + cf));
    const V uc = uat(r), sc = sat(r);
    const float ws = SELF ? wself[r] : 0.0f;
    const float vi = v[r], avi = vnew[r];
    const int e0 = rowptr[r];
    const int e1 = rowptr[r + 1];
    V au = vzero(V{}), as = vzero(V{});
    int e = e0;
    for (; e + 4 <= e1; e += 4) {
      const int64_t c0 = col[e], c1 = col[e + 1], c2 = col[e + 2], c3 = col[e + 3];
      const V u0 = uat(c0), u1 = uat(c1), u2 = uat(c2), u3 = uat(c3);
      const V s0 = sat(c0), s1 = sat(c1), s2 = sat(c2), s3 = sat(c3);
      const float w0 = val[e], w1 = val[e + 1], w2 = val[e + 2], w3 = val[e + 3];
      au = fmac(au, w0, u0);
      as = fmac(as, w0, s0);
      au = fmac(au, w1, u1);
      as = fmac(as, w1, s1);
      au = fmac(au, w2, u2);
      as = fmac(as, w2, s2);
      au = fmac(au, w3, u3);
      as = fmac(as, w3, s3);
    }
    for (; e < e1; ++e) {
      const int64_t cj = col[e];
      const float w = val[e];
      au = fmac(au, w, uat(cj));
      as = fmac(as, w, sat(cj));
    }
    V uo, so;
    gt_push_finish<OBJ>(au, as, uc, sc, t, ws, SELF, a.neg_lr, vi, avi, uo, so);
    __builtin_nontemporal_store(uo, reinterpret_cast<V*>(a.UO + int64_t(r) * a.lduo + cf));
    __builtin_nontemporal_store(so, reinterpret_cast<V*>(a.SO + int64_t(r) * a.ldso + cf));
  }
}

// ----------------------------------------------------------------------------
// gt_csr_xcd_kernel's form for large graphs with non-local neighbours: a
// column tile is W f4 wide and every block of that tile has the same
// blockIdx % 8, so the tile's slabs of U and of S live in ONE XCD's L2
// (placement is a speed assumption only).  One block = (256 / W) x PASSES rows
// of the tile.  Degree-4 rows gather every pass's indices, then every
// neighbour row of both matrices, then the centre and target rows, before any
// arithmetic; other degrees walk their lists 4 at a time.  Rows past the end
// of a ragged block read row n - 1's lists, rows and push-sum weights (valid
// loads) and store nothing.
// ----------------------------------------------------------------------------
template <int W, int PASSES, int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_push_csr_xcd_kernel(GtPush a, int n_rows, uint32_t nrb, uint32_t ntiles,
                                                                   const int32_t* __restrict__ rowptr,
                                                                   const int32_t* __restrict__ col,
                                                                   const float* __restrict__ val,
                                                                   const float* __restrict__ wself,
                                                                   const float* __restrict__ v,
                                                                   const float* __restrict__ vnew) {
  constexpr int ROWS = kThreads / W;
  constexpr int RB = ROWS * PASSES;
  const uint32_t b = blockIdx.x;
  const uint32_t xcd = b & 7u, local = b >> 3;
  const uint32_t tloc = local / nrb, rb = local % nrb;
  const uint32_t ct = tloc * 8 + xcd;
  if (ct >= ntiles) return;
  const int lane_c = threadIdx.x % W, lane_r = threadIdx.x / W;
  const int64_t c = int64_t(ct) * W + lane_c;  // f4 column
  const f4* ub = reinterpret_cast<const f4*>(a.U) + c;
  const f4* sb = reinterpret_cast<const f4*>(a.S) + c;
  const f4* tb = reinterpret_cast<const f4*>(a.T) + c;
  const int64_t lduv = a.ldu / 4, ldsv = a.lds / 4, ldtv = a.ldt / 4;
  int rr[PASSES], rc[PASSES], e0[PASSES], e1[PASSES];
  bool four = true;
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    rr[p] = int(rb) * RB + p * ROWS + lane_r;
    rc[p] = rr[p] < n_rows ? rr[p] : n_rows - 1;
    e0[p] = rowptr[rc[p]];
    e1[p] = rowptr[rc[p] + 1];
    four = four && (e1[p] - e0[p] == 4);
  }
  // the centre rows, the target row, the self weight and the two push-sum
  // weights of every pass: issued ahead of the gathers on either path (clamped
  // rows: valid loads)
  f4 uc[PASSES], sc[PASSES], tv[PASSES];
  float ws[PASSES], vi[PASSES], avi[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    uc[p] = ub[int64_t(rc[p]) * lduv];
    sc[p] = sb[int64_t(rc[p]) * ldsv];
    tv[p] = __builtin_nontemporal_load(tb + int64_t(rc[p]) * ldtv);
    ws[p] = SELF ? wself[rc[p]] : 0.0f;
    vi[p] = v[rc[p]];
    avi[p] = vnew[rc[p]];
  }
  if (four) {
    int cc[PASSES][4];
    float vv[PASSES][4];
#pragma unroll
    for (int p = 0; p < PASSES; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        cc[p][q] = col[e0[p] + q];
        vv[p][q] = val[e0[p] + q];
      }
    f4 us[PASSES][4], ss[PASSES][4];
#pragma unroll
    for (int p = 0; p < PASSES; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        us[p][q] = ub[int64_t(cc[p][q]) * lduv];
        ss[p][q] = sb[int64_t(cc[p][q]) * ldsv];
      }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      if (rr[p] < n_rows) {
        f4 au = f4{0.f, 0.f, 0.f, 0.f}, as = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          au = fmac(au, vv[p][q], us[p][q]);
          as = fmac(as, vv[p][q], ss[p][q]);
        }
        f4 uo, so;
        gt_push_finish<OBJ>(au, as, uc[p], sc[p], tv[p], ws[p], SELF, a.neg_lr, vi[p], avi[p], uo, so);
        __builtin_nontemporal_store(uo, reinterpret_cast<f4*>(a.UO + int64_t(rr[p]) * a.lduo) + c);
        __builtin_nontemporal_store(so, reinterpret_cast<f4*>(a.SO + int64_t(rr[p]) * a.ldso) + c);
      }
    }
    return;
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int r = rr[p];
    if (r < n_rows) {
      f4 au = f4{0.f, 0.f, 0.f, 0.f}, as = f4{0.f, 0.f, 0.f, 0.f};
      int e = e0[p];
      for (; e + 4 <= e1[p]; e += 4) {
        const int64_t c0 = col[e], c1 = col[e + 1], c2 = col[e + 2], c3 = col[e + 3];
        const f4 u0 = ub[c0 * lduv], u1 = ub[c1 * lduv], u2 = ub[c2 * lduv], u3 = ub[c3 * lduv];
        const f4 s0 = sb[c0 * ldsv], s1 = sb[c1 * ldsv], s2 = sb[c2 * ldsv], s3 = sb[c3 * ldsv];
        const float w0 = val[e], w1 = val[e + 1], w2 = val[e + 2], w3 = val[e + 3];
        au = fmac(au, w0, u0);
        as = fmac(as, w0, s0);
        au = fmac(au, w1, u1);
        as = fmac(as, w1, s1);
        au = fmac(au, w2, u2);
        as = fmac(as, w2, s2);
        au = fmac(au, w3, u3);
        as = fmac(as, w3, s3);
      }
      for (; e < e1[p]; ++e) {
        const int64_t cj = col[e];
        const float w = val[e];
        au = fmac(au, w, ub[cj * lduv]);
        as = fmac(as, w, sb[cj * ldsv]);
      }
      f4 uo, so;
      gt_push_finish<OBJ>(au, as, uc[p], sc[p], tv[p], ws[p], SELF, a.neg_lr, vi[p], avi[p], uo, so);
      __builtin_nontemporal_store(uo, reinterpret_cast<f4*>(a.UO + int64_t(r) * a.lduo) + c);
      __builtin_nontemporal_store(so, reinterpret_cast<f4*>(a.SO + int64_t(r) * a.ldso) + c);
    }
  }
}

template <typename V, int OBJ, bool SELF>
void launch_gt_push_csr(const GtPush& a, int n_rows, int64_t c_off, int64_t ncols_v, const int32_t* rowptr,
                        const int32_t* col, const float* val, const float* wself, const float* v, const float* vnew,
                        hipStream_t s) {
  const int64_t n_rg = cdiv(n_rows, kGtPushRows);
  hipLaunchKernelGGL((gt_push_csr_kernel<V, OBJ, SELF>), dim3(static_cast<unsigned>(cdiv(ncols_v, kThreads) * n_rg)),
                     dim3(kThreads), 0, s, a, n_rows, c_off, ncols_v, n_rg, rowptr, col, val, wself, v, vnew);
}

}  // namespace

extern "C" {

int dol_gt_push_csr_f32(const float* U, int64_t ldu, const float* S, int64_t lds, float* UO, int64_t lduo, float* SO,
                        int64_t ldso, int32_t n, int64_t P, const int32_t* rowptr, const int32_t* col,
                        const float* val, const float* self_w, const float* target, int64_t ldt, int32_t objective,
                        float lr, const float* v, float* v_out, hipStream_t s) {
  const char* nm = "dol_gt_push_csr_f32";
  const GtRows m{U, ldu, S, lds, UO, lduo, SO, ldso, target, ldt};
  DOL_CHECKED(m.check(nm, n, P, !rowptr || !col || !val || !v || !v_out));
  if (const int rc = GtRows::objective_ok(nm, objective)) return rc;
  if (v == v_out) return fail(DOL_EINVAL, "%s: v and v_out alias (every v' reads its neighbours' v)", nm);
  const ColSplit cs = split_cols(P, m.vec_ok());
  constexpr int XW = 32, XPASSES = 2;  // XCD-pinned tiles: 512 B of a row, 16 rows per block
  const int64_t n_rg = cdiv(n, kGtPushRows);
  if (mul_sat(cdiv(cs.n4, kThreads), n_rg) > kMaxBlocks || mul_sat(cdiv(cs.tail, kThreads), n_rg) > kMaxBlocks)
    return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const bool use_xcd = cs.n4 >= XW && n >= kGtPushMinXcdRows;
  const int64_t nt = use_xcd ? cs.n4 / XW : 0;
  const int64_t nrb = cdiv(n, (kThreads / XW) * XPASSES);
  if (cdiv(nt, 8) * 8 * nrb > kMaxBlocks * 8) return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const int64_t done4 = nt * XW;
  const GtPush a{U, ldu, S, lds, UO, lduo, SO, ldso, target, ldt, -lr};
  dispatch([&](auto obj, auto self) {
    constexpr int OBJ = decltype(obj)::value;
    constexpr bool SELF = decltype(self)::value;
    // v' = C v first: the main kernels read it, ordered after it on the stream
    hipLaunchKernelGGL((gt_push_v_kernel<SELF>), dim3(static_cast<unsigned>(cdiv(n, kThreads))), dim3(kThreads), 0, s,
                       n, rowptr, col, val, self_w, v, v_out);
    if (nt > 0)
      hipLaunchKernelGGL((gt_push_csr_xcd_kernel<XW, XPASSES, OBJ, SELF>),
                         dim3(static_cast<unsigned>(cdiv(nt, 8) * 8 * nrb)), dim3(kThreads), 0, s, a, n,
                         static_cast<uint32_t>(nrb), static_cast<uint32_t>(nt), rowptr, col, val, self_w, v, v_out);
    if (cs.n4 > done4)
      launch_gt_push_csr<f4, OBJ, SELF>(a, n, done4 * 4, cs.n4 - done4, rowptr, col, val, self_w, v, v_out, s);
    if (cs.tail > 0)
      launch_gt_push_csr<float, OBJ, SELF>(a, n, cs.n4 * 4, cs.tail, rowptr, col, val, self_w, v, v_out, s);
  }, Ints<0, 1>{objective}, Bool{self_w != nullptr});
  return check_launch(nm);
}

}  // extern "C"
