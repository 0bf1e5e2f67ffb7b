// grad_rounds.hip — the gradient-tracking round of gt_csr.hip with the gradient
// FED as a row matrix instead of computed in the kernel from a target row:
//   dol_gt_grad_csr_f32   DIGing with the tracker update at the front of the
//                         round, s_k = W s_{k-1} + G_k - G_{k-1}, then
//                         x_{k+1} = W x_k - lr s_k
// for agents whose gradients something else computes (BatchedMLP's
// forward_backward writes them into the bank's grad rows; autograd into bank
// rows for the CNN agents).  Its EXTRA sibling, dol_extra_grad_csr_f32, is an
// epilogue of the CSR mix and lives beside dol_extra_csr_f32 in csr.hip
// (ExtraEpi with kObjGradRow, dol_launch.h): it needs no kernel of its own.
//
// Layout as gt_csr.hip: agent i's vector is row i of a row-major fp32 matrix.
// X and S are gathered through ONE read of rowptr / col / val per row; the
// gradient rows g_i (this round's) and gprev_i (last round's) are the centre
// row's only.  For every row i and column c, all fp32, each operation rounded
// once (-ffp-contract=off):
//   ax = sum_e val[e] * x[col[e]]      (+0 start, ascending e: fmac())     as = the same over s
// and then gt_grad_finish (dol_launch.h) with d = self_w[i]:
//   self:  ax = fl(ax + fl(d x_i));  as = fl(as + fl(d s_i))
//   s' = fl(fl(as + g_i) - gprev_i);   x' = fma(-lr, s', ax)
// x' takes the agent's own NEW tracker, so the round is one pass; from S = 0 and
// Gprev = 0 the first round gives s = G, so there is no separate start.
// separable_grad is not called.  Without self weights the centre rows of X and
// S are not needed and are not loaded.
//
// Why kernels of its own and not a third tag of gt_csr.hip's body: the fed
// round carries two read-once row matrices where that body carries one (GtCsr
// is a kernel argument of every instantiation there, and the tag must stay
// stateless: gt_csr.hip's header), so sharing would change the arguments, and
// with them the emitted code, of the six existing kernels.  The three forms,
// the column split, the launch-size refusals and the clamped ragged rows are
// gt_csr.hip's: 512-B XCD-pinned tiles from 512 rows, 4 KiB f4 tiles for small
// graphs and the f4 columns the pinned tiles leave over, scalar columns for P %
// 4 and for rows that are not 16-B aligned.
//
// Policies: the gathered rows and (with self weights) the centre rows of X and
// S load with the default policy; G and Gprev are read once and load
// nontemporal; both stores are nontemporal.  Six streams to dol_gt_csr_f32's
// five.
//
// Resource usage, from the compiler's kernel-resource-usage remarks (gfx950,
// -O3; occupancy in waves per SIMD; no instantiation uses scratch or LDS):
//   kernel                              VGPRs: no self / self   scratch   occupancy
//   gt_grad_csr_xcd_kernel<32, 2>       106 / 122               0         4 / 4
//   gt_grad_csr_kernel<f4>              76 / 84                 0         6 / 5
//   gt_grad_csr_kernel<float>           40 / 42                 0         8 / 8
// The pinned degree-4 path keeps gt_csr_xcd_kernel's 4 waves per SIMD (at most
// 128 VGPRs) with the two gradient rows loaded AHEAD of the gathers, as that
// kernel loads its target row: with self weights it holds one more centre f4
// per pass than gt_csr_xcd_kernel (x, s, g, gprev against x, s, t) and lands on
// that kernel's 122; without them it holds one fewer.  Loading G and Gprev after
// the gather arithmetic instead was compiled as well (120 / 102 VGPRs, the same
// 4 waves): no occupancy to recover, so the loads stay ahead, where their
// latency overlaps the gathers'.  The small-n f4 kernel with self weights is at
// 84 VGPRs, 5 waves per SIMD where gt_csr_kernel<GtPlain, f4> has 6 (78-80): it
// runs below 512 rows and on at most 31 left-over f4 columns of the pinned
// form, and was left as it is.
#include "dol_launch.h"

namespace {
constexpr int kThreads = 256;  // 4 waves of 64
constexpr int kRows = 16;  // rows per block of gt_grad_csr_kernel (gt_csr.hip's kRows)
constexpr int kMinXcdRows = 512;  // the XCD-pinned form from this many rows (csr.hip's rule)

struct GtGradCsr {
  const float* X; int64_t ldx;
  const float* S; int64_t lds;
  float* XO; int64_t ldxo;
  float* SO; int64_t ldso;
  const float* G; int64_t ldg;
  const float* GP; int64_t ldgp;
  float neg_lr;
};

// ----------------------------------------------------------------------------
// 4 KiB column tiles (V = f4) or 1 KiB of scalar columns (V = float), kRows rows
// per block, row group fastest: gt_csr_kernel's geometry.  c_off: the first
// element column of this launch.
// ----------------------------------------------------------------------------
template <typename V, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_grad_csr_kernel(GtGradCsr a, int n_rows, int64_t c_off,
                                                               int64_t ncols_v, int64_t n_row_groups,
                                                               const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col,
                                                               const float* __restrict__ val,
                                                               const float* __restrict__ wself) {
  constexpr int VW = Vec<V>::W;
  const int64_t b = blockIdx.x;
  const int rg = static_cast<int>(b % n_row_groups);
  const int64_t c = (b / n_row_groups) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  const int r0 = rg * kRows;
  const int r1 = min(r0 + kRows, n_rows);
  const int64_t cf = c_off + c * VW;  // element column
  const float* xb = a.X + cf;
  const float* sb = a.S + cf;
  auto xat = [&](int64_t r) { return *reinterpret_cast<const V*>(xb + r * a.ldx); };
  auto sat = [&](int64_t r) { return *reinterpret_cast<const V*>(sb + r * a.lds); };
  for (int r = r0; r < r1; ++r) {
    const V g = ldv<V, sizeof(V) == 16>(reinterpret_cast<const V*>(a.G + int64_t(r) * a.ldg + cf));
    const V gp = ldv<V, sizeof(V) == 16>(reinterpret_cast<const V*>(a.GP + int64_t(r) * a.ldgp + cf));
    V xc = vzero(V{}), sc = vzero(V{});
    float ws = 0.0f;
    if constexpr (SELF) {
      xc = xat(r);
      sc = sat(r);
      ws = wself[r];
    }
    const int e0 = rowptr[r];
    const int e1 = rowptr[r + 1];
    V ax = vzero(V{}), as = vzero(V{});
    int e = e0;
    for (; e + 4 <= e1; e += 4) {
      const int64_t c0 = col[e], c1 = col[e + 1], c2 = col[e + 2], c3 = col[e + 3];
      const V x0 = xat(c0), x1 = xat(c1), x2 = xat(c2), x3 = xat(c3);
      const V s0 = sat(c0), s1 = sat(c1), s2 = sat(c2), s3 = sat(c3);
      const float w0 = val[e], w1 = val[e + 1], w2 = val[e + 2], w3 = val[e + 3];
      ax = fmac(ax, w0, x0);
      as = fmac(as, w0, s0);
      ax = fmac(ax, w1, x1);
      as = fmac(as, w1, s1);
      ax = fmac(ax, w2, x2);
      as = fmac(as, w2, s2);
      ax = fmac(ax, w3, x3);
      as = fmac(as, w3, s3);
    }
    for (; e < e1; ++e) {
      const int64_t cj = col[e];
      const float w = val[e];
      ax = fmac(ax, w, xat(cj));
      as = fmac(as, w, sat(cj));
    }
    V xo, so;
    gt_grad_finish(ax, as, xc, sc, g, gp, ws, SELF, a.neg_lr, xo, so);
    __builtin_nontemporal_store(xo, reinterpret_cast<V*>(a.XO + int64_t(r) * a.ldxo + cf));
    __builtin_nontemporal_store(so, reinterpret_cast<V*>(a.SO + int64_t(r) * a.ldso + cf));
  }
}

// ----------------------------------------------------------------------------
// XCD-pinned form, gt_csr_xcd_kernel's geometry: a column tile is W f4 wide and
// every block of that tile has the same blockIdx % 8, so the tile's slabs of X
// and of S live in ONE XCD's L2.  Placement is a speed assumption only.  One
// block = (256 / W) x PASSES rows of the tile.  Degree-4 rows gather every
// pass's indices, then every neighbour row of both matrices, before any
// arithmetic; other degrees walk their lists 4 at a time.  Rows past the end of
// a ragged block read row n - 1's lists and rows (valid loads) and store
// nothing.
// ----------------------------------------------------------------------------
template <int W, int PASSES, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_grad_csr_xcd_kernel(GtGradCsr a, int n_rows, uint32_t nrb,
                                                                   uint32_t ntiles,
                                                                   const int32_t* __restrict__ rowptr,
                                                                   const int32_t* __restrict__ col,
                                                                   const float* __restrict__ val,
                                                                   const float* __restrict__ wself) {
  constexpr int ROWS = kThreads / W;
  constexpr int RB = ROWS * PASSES;
  const uint32_t b = blockIdx.x;
  const uint32_t xcd = b & 7u, local = b >> 3;
  const uint32_t tloc = local / nrb, rb = local % nrb;
  const uint32_t ct = tloc * 8 + xcd;
  if (ct >= ntiles) return;
  const int lane_c = threadIdx.x % W, lane_r = threadIdx.x / W;
  const int64_t c = int64_t(ct) * W + lane_c;  // f4 column
  const f4* xb = reinterpret_cast<const f4*>(a.X) + c;
  const f4* sb = reinterpret_cast<const f4*>(a.S) + c;
  const f4* gb = reinterpret_cast<const f4*>(a.G) + c;
  const f4* pb = reinterpret_cast<const f4*>(a.GP) + c;
  const int64_t ldxv = a.ldx / 4, ldsv = a.lds / 4, ldgv = a.ldg / 4, ldpv = a.ldgp / 4;
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
  // the gradient rows of every pass, and with self weights the centre rows and
  // the weight: issued ahead of the gathers on either path (clamped rows: valid
  // loads)
  f4 xc[PASSES], sc[PASSES], gv[PASSES], pv[PASSES];
  float ws[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    xc[p] = sc[p] = f4{0.f, 0.f, 0.f, 0.f};
    ws[p] = 0.0f;
    if constexpr (SELF) {
      xc[p] = xb[int64_t(rc[p]) * ldxv];
      sc[p] = sb[int64_t(rc[p]) * ldsv];
      ws[p] = wself[rc[p]];
    }
    gv[p] = __builtin_nontemporal_load(gb + int64_t(rc[p]) * ldgv);
    pv[p] = __builtin_nontemporal_load(pb + int64_t(rc[p]) * ldpv);
  }
  auto finish = [&](int p, f4 ax, f4 as) {
    f4 xo, so;
    gt_grad_finish(ax, as, xc[p], sc[p], gv[p], pv[p], ws[p], SELF, a.neg_lr, xo, so);
    __builtin_nontemporal_store(xo, reinterpret_cast<f4*>(a.XO + int64_t(rr[p]) * a.ldxo) + c);
    __builtin_nontemporal_store(so, reinterpret_cast<f4*>(a.SO + int64_t(rr[p]) * a.ldso) + c);
  };
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
    f4 xs[PASSES][4], ss[PASSES][4];
#pragma unroll
    for (int p = 0; p < PASSES; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xs[p][q] = xb[int64_t(cc[p][q]) * ldxv];
        ss[p][q] = sb[int64_t(cc[p][q]) * ldsv];
      }
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      if (rr[p] < n_rows) {
        f4 ax = f4{0.f, 0.f, 0.f, 0.f}, as = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ax = fmac(ax, vv[p][q], xs[p][q]);
          as = fmac(as, vv[p][q], ss[p][q]);
        }
        finish(p, ax, as);
      }
    }
    return;
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    if (rr[p] < n_rows) {
      f4 ax = f4{0.f, 0.f, 0.f, 0.f}, as = f4{0.f, 0.f, 0.f, 0.f};
      int e = e0[p];
      for (; e + 4 <= e1[p]; e += 4) {
        const int64_t c0 = col[e], c1 = col[e + 1], c2 = col[e + 2], c3 = col[e + 3];
        const f4 x0 = xb[c0 * ldxv], x1 = xb[c1 * ldxv], x2 = xb[c2 * ldxv], x3 = xb[c3 * ldxv];
        const f4 s0 = sb[c0 * ldsv], s1 = sb[c1 * ldsv], s2 = sb[c2 * ldsv], s3 = sb[c3 * ldsv];
        const float w0 = val[e], w1 = val[e + 1], w2 = val[e + 2], w3 = val[e + 3];
        ax = fmac(ax, w0, x0);
        as = fmac(as, w0, s0);
        ax = fmac(ax, w1, x1);
        as = fmac(as, w1, s1);
        ax = fmac(ax, w2, x2);
        as = fmac(as, w2, s2);
        ax = fmac(ax, w3, x3);
        as = fmac(as, w3, s3);
      }
      for (; e < e1[p]; ++e) {
        const int64_t cj = col[e];
        const float w = val[e];
        ax = fmac(ax, w, xb[cj * ldxv]);
        as = fmac(as, w, sb[cj * ldsv]);
      }
      finish(p, ax, as);
    }
  }
}

template <typename V, bool SELF>
void launch_gt_grad_csr(const GtGradCsr& a, int n_rows, int64_t c_off, int64_t ncols_v, const int32_t* rowptr,
                        const int32_t* col, const float* val, const float* wself, hipStream_t s) {
  const int64_t n_rg = cdiv(n_rows, kRows);
  hipLaunchKernelGGL((gt_grad_csr_kernel<V, SELF>), dim3(static_cast<unsigned>(cdiv(ncols_v, kThreads) * n_rg)),
                     dim3(kThreads), 0, s, a, n_rows, c_off, ncols_v, n_rg, rowptr, col, val, wself);
}

}  // namespace

extern "C" {

int dol_gt_grad_csr_f32(const float* X, int64_t ldx, const float* S, int64_t lds, float* XO, int64_t ldxo, float* SO,
                        int64_t ldso, int32_t n, int64_t P, const int32_t* rowptr, const int32_t* col,
                        const float* val, const float* self_w, const float* G, int64_t ldg, const float* Gprev,
                        int64_t ldgp, float lr, hipStream_t s) {
  const char* nm = "dol_gt_grad_csr_f32";
  DOL_DIMS_OK(nm, ldx, lds, ldxo, ldso, ldg, ldgp, P);
  // dol_gt_csr_f32's rules (GtRows::check) with G and Gprev in target's place
  const bool alias = X == S || X == XO || X == SO || S == XO || S == SO || XO == SO;
  DOL_CHECKED(check_rows(nm, n < 0 || P < 0, n == 0 || P == 0,
                         !X || !S || !XO || !SO || !G || !Gprev || !rowptr || !col || !val,
                         ldx < P || lds < P || ldxo < P || ldso < P || ldg < P || ldgp < P, alias,
                         "X, S, XO, SO alias (the Jacobi update of x and s needs four buffers)"));
  if (G == XO || G == SO || Gprev == XO || Gprev == SO)
    return fail(DOL_EINVAL, "%s: G or Gprev aliases XO or SO (the gradient rows are read while the outputs are written)",
                nm);
  const bool vec_ok = row_vec_ok(X, ldx) && row_vec_ok(S, lds) && row_vec_ok(XO, ldxo) && row_vec_ok(SO, ldso) &&
                      row_vec_ok(G, ldg) && row_vec_ok(Gprev, ldgp);
  const ColSplit cs = split_cols(P, vec_ok);
  constexpr int XW = 32, XPASSES = 2;  // XCD-pinned tiles: 512 B of a row, 16 rows per block
  const int64_t n_rg = cdiv(n, kRows);
  if (mul_sat(cdiv(cs.n4, kThreads), n_rg) > kMaxBlocks || mul_sat(cdiv(cs.tail, kThreads), n_rg) > kMaxBlocks)
    return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const bool use_xcd = cs.n4 >= XW && n >= kMinXcdRows;
  const int64_t nt = use_xcd ? cs.n4 / XW : 0;
  const int64_t nrb = cdiv(n, (kThreads / XW) * XPASSES);
  if (cdiv(nt, 8) * 8 * nrb > kMaxBlocks * 8) return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const int64_t done4 = nt * XW;
  const GtGradCsr a{X, ldx, S, lds, XO, ldxo, SO, ldso, G, ldg, Gprev, ldgp, -lr};
  dispatch([&](auto self) {
    constexpr bool SELF = decltype(self)::value;
    if (nt > 0)
      hipLaunchKernelGGL((gt_grad_csr_xcd_kernel<XW, XPASSES, SELF>),
                         dim3(static_cast<unsigned>(cdiv(nt, 8) * 8 * nrb)), dim3(kThreads), 0, s, a, n,
                         static_cast<uint32_t>(nrb), static_cast<uint32_t>(nt), rowptr, col, val, self_w);
    if (cs.n4 > done4) launch_gt_grad_csr<f4, SELF>(a, n, done4 * 4, cs.n4 - done4, rowptr, col, val, self_w, s);
    if (cs.tail > 0) launch_gt_grad_csr<float, SELF>(a, n, cs.n4 * 4, cs.tail, rowptr, col, val, self_w, s);
  }, Bool{self_w != nullptr});
  return check_launch(nm);
}

}  // extern "C"
