// gt_ring.hip — one gradient-tracking round (DIGing / NEXT) on the agent-major
// ring in one HBM pass: dol_gt_ring_f32, the ring sibling of dol_gt_csr_pm_f32
// (pmajor.hip), and dol_gt_ring_edges_f32, the two boundary rows of a sharded
// block.  Its own translation unit, so ring.o and its pinned kernels stay as
// they are.
//
// Layout as ring.hip: agent k's vector is row k of a row-major fp32 matrix.
// Two row matrices, the parameters X and the trackers S, go through ONE ring
// stencil; the target rows T ride along.  For every row r and column c, all
// fp32, each operation rounded once (-ffp-contract=off):
//   ax = fl(fl(+0 + fl(wp[r] x[r-1])) + fl(wn[r] x[r+1]))     axpy0, as dol_mix_ring_f32
//   as = the same over s
// and then gt_finish (dol_launch.h) with d = w_self[r], the lane that
// dol_gt_csr_pm_f32 runs too: the same bits as that round on the ring's CSR
// with the same self weights, because the CSR sums the two neighbours in
// ascending column order, here it is previous then next, and fl(fl(+0 + a) + b)
// commutes in a and b (dol_mix_ring_f32's argument).  The Epi hook of
// ring_mix_dma_kernel cannot say this: an epilogue sees one mixed value, this
// round needs two and the centre rows of both.
#include "dol_launch.h"

namespace {
constexpr int kThreads = 256;  // 4 waves of 64
constexpr int kGtTailRows = 4;  // rows per block of the scalar kernel
constexpr int kGtRows = 4;      // R of gt_ring_dma_kernel
constexpr int kGtPanel = 512;   // column tiles per panel of its block order (a multiple of 8)

template <int OBJ, bool SELF>
__device__ __forceinline__ void gt_ring_lane(float xp, float x, float xn, float sp, float s, float sn, float t,
                                             float wp, float wn, float ws, float neg_lr, float& xo, float& so) {
  gt_finish<OBJ>(axpy0(wp, xp, wn, xn), axpy0(wp, sp, wn, sn), x, s, t, ws, SELF, neg_lr, xo, so);
}

struct GtRing {
  const float* X; int64_t ldx;
  const float* S; int64_t lds;
  float* XO; int64_t ldxo;
  float* SO; int64_t ldso;
  const float* T; int64_t ldt;
  const float* xhp; const float* xhn;  // row -1 and row n_rows of X (the wrap-around rows without halos)
  const float* shp; const float* shn;  // the same of S
  float neg_lr;
  // row r of X / of S, r in [-1, n]: the matrix row, or the halo on its side
  __device__ __forceinline__ const float* xrow(int r, int n) const { return pick(X, ldx, xhp, xhn, r, n); }
  __device__ __forceinline__ const float* srow(int r, int n) const { return pick(S, lds, shp, shn, r, n); }
  static __device__ __forceinline__ const float* pick(const float* M, int64_t ld, const float* hp, const float* hn,
                                                      int r, int n) {
    return (r < 0) ? hp : (r >= n ? hn : M + int64_t(r) * ld);
  }
};
// (the weight vectors are kernel arguments of their own, const __restrict__: the
// compiler then reads them with scalar loads, ahead of the DMA wait)

// ----------------------------------------------------------------------------
// LDS-DMA form (the float4 path), a sibling of ring_mix_dma_kernel: one
// workgroup = one column tile (256 lanes x f4) x R rows.  Each wave moves its
// 1 KiB quarter of the tile's R + 2 rows of X and of S straight into LDS with
// global_load_lds_dwordx4, waits on its own vmcnt, reads its lanes back.  No
// barrier: a wave only reads what it loaded.  The four window rows the
// vertically neighbouring tiles read too (k = 0, 1, R, R + 1) load with the
// default policy so that the second read hits L2; the R - 2 rows between them,
// the target rows and both stores are nontemporal (ring.hip's NTI finding, and
// DgdEpi's for the target rows).  LDS per workgroup: 4 waves x 2 matrices x
// (R + 2) KiB = 48 KiB at R = 4, three workgroups per CU, 96 per XCD.
// Block order.  ring_mix_dma_kernel runs column tile fastest and finds its halo
// rows in L2 because a whole row of tiles (1024 at P = 2^20) is co-resident;
// with twice the LDS here 768 are, and in that order this kernel fetched
// 1.14-1.20 x its algorithmic read (FETCH_SIZE x 2 against 3 N P 4 at
// 1024 x 2^20): about half of the halo re-reads missed.  So the column tiles
// go in panels of kGtPanel: the dispatcher deals blocks round-robin over the 8
// XCDs, a vertical neighbour is kGtPanel / 8 = 64 blocks later on the same XCD
// (kGtPanel % 8 == 0), inside the 96 resident there.  Measured at 1024 x 2^20,
// ld = 2^20 + 2048, one box, (a) / dgd_ring pairs and the read ratio
// (tools/gt_ab.py, profiles/gt_ring_ab.jsonl): no panels 1.017 / 1.147;
// 64 1.167 / 1.0014; 128 1.175 / 1.0015; 256 1.11 / 1.0014; 512 0.965-1.008 /
// 1.0017; 768 1.05 / 1.035; 1024 1.02 / 1.13.  Narrow panels hit L2 as well but
// stream shorter runs of each row.
// R = 8 (80 KiB, two workgroups per CU, half the halo re-reads) lost on both
// sizes, before the panels: 4.45-5.00 vs 4.09 ms at 1024 x 2^20 (ld = 2^20),
// 29.16 vs 27.68-28.19 at 8192 x 2^20 (ld = 2^20 + 2048), processes alternating.
// Every load stays inside its matrix: window rows clamp to min(r0 - 1 + k, r1)
// (row r1 <= n_rows exists: the next row or the next halo), target rows to
// min(r0 + k, r1 - 1).
// ----------------------------------------------------------------------------
template <int R, int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_ring_dma_kernel(GtRing a, const float* __restrict__ wprev,
                                                               const float* __restrict__ wnext,
                                                               const float* __restrict__ wself, int n_rows,
                                                               int64_t ncols_v, uint32_t nct, uint32_t n_row_tiles) {
  __shared__ __attribute__((aligned(16))) float lds[kThreads / 64][2][R + 2][256];
  // Block order: panels of kGtPanel column tiles; inside a panel the row tiles in
  // order, and inside a row tile the panel's column tiles (the last panel may be
  // narrower).
  constexpr uint32_t panel = kGtPanel;
  const uint32_t b = blockIdx.x;
  const uint32_t full = nct / panel * panel;               // column tiles in whole panels
  const uint32_t pn = full ? panel * n_row_tiles : 1u;      // blocks per whole panel (grids are < 2^24 blocks)
  const bool whole = b < full * n_row_tiles;
  const uint32_t w = whole ? panel : max(nct - full, 1u);   // this panel's width
  const uint32_t in_panel = whole ? b % pn : b - full * n_row_tiles;
  const uint32_t ct = (whole ? b / pn * panel : full) + in_panel % w;
  const uint32_t rt = in_panel / w;
  const int r0 = static_cast<int>(rt) * R;
  const int r1 = min(r0 + R, n_rows);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t c = int64_t(ct) * kThreads + threadIdx.x;  // f4 column
  if (c >= ncols_v) return;
#pragma unroll
  for (int k = 0; k < R + 2; ++k) {
    const int r = min(r0 - 1 + k, r1);
    if (k >= 2 && k < R) {  // rows no other tile reads: nontemporal
      __builtin_amdgcn_global_load_lds(DOL_GPTR(a.xrow(r, n_rows) + 4 * c), DOL_LPTR(&lds[wave][0][k][0]), 16, 0, 2);
      __builtin_amdgcn_global_load_lds(DOL_GPTR(a.srow(r, n_rows) + 4 * c), DOL_LPTR(&lds[wave][1][k][0]), 16, 0, 2);
    } else {
      __builtin_amdgcn_global_load_lds(DOL_GPTR(a.xrow(r, n_rows) + 4 * c), DOL_LPTR(&lds[wave][0][k][0]), 16, 0, 0);
      __builtin_amdgcn_global_load_lds(DOL_GPTR(a.srow(r, n_rows) + 4 * c), DOL_LPTR(&lds[wave][1][k][0]), 16, 0, 0);
    }
  }
  f4 tv[R];  // the target rows and the weights ride with the DMA
  float wp[R], wn[R], ws[R];
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int r = min(r0 + k, r1 - 1);
    tv[k] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(a.T + int64_t(r) * a.ldt) + c);
    wp[k] = wprev[r];
    wn[k] = wnext[r];
    ws[k] = SELF ? wself[r] : 0.0f;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f4 xv[R + 2], sv[R + 2];
#pragma unroll
  for (int k = 0; k < R + 2; ++k) {
    xv[k] = *reinterpret_cast<const f4*>(&lds[wave][0][k][lane * 4]);
    sv[k] = *reinterpret_cast<const f4*>(&lds[wave][1][k][lane * 4]);
  }
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int r = r0 + k;
    if (r < r1) {
      f4 xo, so;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float xe, se;
        gt_ring_lane<OBJ, SELF>(xv[k][j], xv[k + 1][j], xv[k + 2][j], sv[k][j], sv[k + 1][j], sv[k + 2][j], tv[k][j],
                                wp[k], wn[k], ws[k], a.neg_lr, xe, se);
        xo[j] = xe;
        so[j] = se;
      }
      __builtin_nontemporal_store(xo, reinterpret_cast<f4*>(a.XO + int64_t(r) * a.ldxo) + c);
      __builtin_nontemporal_store(so, reinterpret_cast<f4*>(a.SO + int64_t(r) * a.ldso) + c);
    }
  }
}

// ----------------------------------------------------------------------------
// Scalar columns: the P % 4 tail, or every column when a row base is not 16-B
// aligned.  One workgroup = 256 columns from c_off on x kGtTailRows rows; the
// three-point window of both matrices is carried down the rows in registers,
// so each row is loaded once per block.  Rows r0 - 1 .. r1 only (r1 <= n_rows).
// ----------------------------------------------------------------------------
template <int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_ring_kernel(GtRing a, const float* __restrict__ wprev,
                                                           const float* __restrict__ wnext,
                                                           const float* __restrict__ wself, int n_rows, int64_t c_off,
                                                           int64_t ncols, int64_t n_col_tiles) {
  const uint32_t b = blockIdx.x;
  const uint32_t nct = static_cast<uint32_t>(n_col_tiles);
  const int64_t c = int64_t(b % nct) * kThreads + threadIdx.x;
  if (c >= ncols) return;
  const int r0 = static_cast<int>(b / nct) * kGtTailRows;
  const int r1 = min(r0 + kGtTailRows, n_rows);
  const int64_t cf = c_off + c;
  auto xat = [&](int r) { return a.xrow(r, n_rows)[cf]; };
  auto sat = [&](int r) { return a.srow(r, n_rows)[cf]; };
  float xp = xat(r0 - 1), x = xat(r0), sp = sat(r0 - 1), s = sat(r0);
  for (int r = r0; r < r1; ++r) {
    const float xn = xat(r + 1), sn = sat(r + 1);
    const float t = a.T[int64_t(r) * a.ldt + cf];
    float xo, so;
    gt_ring_lane<OBJ, SELF>(xp, x, xn, sp, s, sn, t, wprev[r], wnext[r], SELF ? wself[r] : 0.0f, a.neg_lr, xo, so);
    a.XO[int64_t(r) * a.ldxo + cf] = xo;
    a.SO[int64_t(r) * a.ldso + cf] = so;
    xp = x, x = xn, sp = s, s = sn;
  }
}

// ----------------------------------------------------------------------------
// The two boundary rows of a sharded ring block in ONE launch (the multi-GPU
// round, dolhip.parallel_gt.sharded_ring_gt_step: the interior rows run while
// the halo rows of X and S travel, then these two), the sibling of
// ring_edges_kernel: blockIdx.y = 0 -> row 0 (previous rows = the two prev
// halos), 1 -> row n_rows - 1 (next rows = the two next halos); with
// n_rows == 1 only y = 0 runs and uses all four halos, with n_rows == 2 each
// edge row's inner neighbour is the other edge row.  V = f4 over the 16-B
// columns, float from c_off on for the scalar ones.  The lane is gt_ring_lane,
// so the bits are dol_gt_ring_f32's.  Plain loads and stores: two rows of a
// block, nothing to keep out of L2.
// ----------------------------------------------------------------------------
template <typename V, int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_ring_edges_kernel(GtRing a, const float* __restrict__ wprev,
                                                                 const float* __restrict__ wnext,
                                                                 const float* __restrict__ wself, int n_rows,
                                                                 int64_t c_off, int64_t ncols_v) {
  const int64_t c = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  const int r = blockIdx.y == 0 ? 0 : n_rows - 1;
  auto at = [&](const float* row) { return reinterpret_cast<const V*>(row + c_off)[c]; };
  const V xp = at(a.xrow(r - 1, n_rows)), x = at(a.xrow(r, n_rows)), xn = at(a.xrow(r + 1, n_rows));
  const V sp = at(a.srow(r - 1, n_rows)), s = at(a.srow(r, n_rows)), sn = at(a.srow(r + 1, n_rows));
  const V t = at(a.T + int64_t(r) * a.ldt);
  const float wp = wprev[r], wn = wnext[r], ws = SELF ? wself[r] : 0.0f;
  V xo, so;
  if constexpr (Vec<V>::W == 1) {
    gt_ring_lane<OBJ, SELF>(xp, x, xn, sp, s, sn, t, wp, wn, ws, a.neg_lr, xo, so);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xe, se;
      gt_ring_lane<OBJ, SELF>(xp[j], x[j], xn[j], sp[j], s[j], sn[j], t[j], wp, wn, ws, a.neg_lr, xe, se);
      xo[j] = xe;
      so[j] = se;
    }
  }
  reinterpret_cast<V*>(a.XO + int64_t(r) * a.ldxo + c_off)[c] = xo;
  reinterpret_cast<V*>(a.SO + int64_t(r) * a.ldso + c_off)[c] = so;
}

}  // namespace

extern "C" {

int dol_gt_ring_f32(const float* X, int64_t ldx, const float* S, int64_t lds, float* XO, int64_t ldxo, float* SO,
                    int64_t ldso, int32_t n_rows, int64_t P, const float* x_halo_prev, const float* x_halo_next,
                    const float* s_halo_prev, const float* s_halo_next, const float* w_prev, const float* w_next,
                    const float* w_self, const float* target, int64_t ldt, int32_t objective, float lr,
                    hipStream_t s) {
  const char* nm = "dol_gt_ring_f32";
  const GtRows m{X, ldx, S, lds, XO, ldxo, SO, ldso, target, ldt};
  DOL_CHECKED(m.check(nm, n_rows, P, !w_prev || !w_next));
  const int n_halos = (x_halo_prev != nullptr) + (x_halo_next != nullptr) + (s_halo_prev != nullptr) +
                      (s_halo_next != nullptr);
  if (n_halos != 0 && n_halos != 4) return fail(DOL_EINVAL, "%s: pass all four halos or none", nm);
  if (n_halos == 0) {
    if (n_rows < 3) return fail(DOL_EINVAL, "%s: wrap-around ring needs n_rows >= 3", nm);
    x_halo_prev = X + int64_t(n_rows - 1) * ldx;
    x_halo_next = X;
    s_halo_prev = S + int64_t(n_rows - 1) * lds;
    s_halo_next = S;
  }
  if (const int rc = GtRows::objective_ok(nm, objective)) return rc;
  const bool vec_ok = m.vec_ok() && aligned16(x_halo_prev) && aligned16(x_halo_next) && aligned16(s_halo_prev) &&
                      aligned16(s_halo_next);
  const ColSplit cs = split_cols(P, vec_ok);
  constexpr int R = kGtRows;
  const int64_t nct4 = cdiv(cs.n4, kThreads), nctt = cdiv(cs.tail, kThreads);
  if (mul_sat(nct4, cdiv(n_rows, R)) > kMaxBlocks || mul_sat(nctt, cdiv(n_rows, kGtTailRows)) > kMaxBlocks)
    return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const GtRing a{X, ldx, S, lds, XO, ldxo, SO, ldso, target, ldt, x_halo_prev, x_halo_next, s_halo_prev, s_halo_next,
                 -lr};
  dispatch([&](auto obj, auto self) {
    constexpr int OBJ = decltype(obj)::value;
    constexpr bool SELF = decltype(self)::value;
    if (cs.n4 > 0)
      hipLaunchKernelGGL((gt_ring_dma_kernel<R, OBJ, SELF>), dim3(static_cast<unsigned>(nct4 * cdiv(n_rows, R))),
                         dim3(kThreads), 0, s, a, w_prev, w_next, w_self, n_rows, cs.n4, static_cast<uint32_t>(nct4),
                         static_cast<uint32_t>(cdiv(n_rows, R)));
    if (cs.tail > 0)
      hipLaunchKernelGGL((gt_ring_kernel<OBJ, SELF>), dim3(static_cast<unsigned>(nctt * cdiv(n_rows, kGtTailRows))),
                         dim3(kThreads), 0, s, a, w_prev, w_next, w_self, n_rows, cs.n4 * 4, cs.tail, nctt);
  }, Ints<0, 1>{objective}, Bool{w_self != nullptr});
  return check_launch(nm);
}

int dol_gt_ring_edges_f32(const float* X, int64_t ldx, const float* S, int64_t lds, float* XO, int64_t ldxo, float* SO,
                          int64_t ldso, int32_t n_rows, int64_t P, const float* x_halo_prev,
                          const float* x_halo_next, const float* s_halo_prev, const float* s_halo_next,
                          const float* w_prev, const float* w_next, const float* w_self, const float* target,
                          int64_t ldt, int32_t objective, float lr, hipStream_t s) {
  const char* nm = "dol_gt_ring_edges_f32";
  const GtRows m{X, ldx, S, lds, XO, ldxo, SO, ldso, target, ldt};
  DOL_CHECKED(m.check(nm, n_rows, P, !w_prev || !w_next || !x_halo_prev || !x_halo_next || !s_halo_prev ||
                                         !s_halo_next));
  if (const int rc = GtRows::objective_ok(nm, objective)) return rc;
  const bool vec_ok = m.vec_ok() && aligned16(x_halo_prev) && aligned16(x_halo_next) && aligned16(s_halo_prev) &&
                      aligned16(s_halo_next);
  const ColSplit cs = split_cols(P, vec_ok);
  const int64_t nct4 = cdiv(cs.n4, kThreads), nctt = cdiv(cs.tail, kThreads);
  if (nct4 > kMaxBlocks || nctt > kMaxBlocks) return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const unsigned ny = n_rows == 1 ? 1u : 2u;
  const GtRing a{X, ldx, S, lds, XO, ldxo, SO, ldso, target, ldt, x_halo_prev, x_halo_next, s_halo_prev, s_halo_next,
                 -lr};
  dispatch([&](auto obj, auto self) {
    constexpr int OBJ = decltype(obj)::value;
    constexpr bool SELF = decltype(self)::value;
    if (cs.n4 > 0)
      hipLaunchKernelGGL((gt_ring_edges_kernel<f4, OBJ, SELF>), dim3(static_cast<unsigned>(nct4), ny), dim3(kThreads),
                         0, s, a, w_prev, w_next, w_self, n_rows, int64_t(0), cs.n4);
    if (cs.tail > 0)
      hipLaunchKernelGGL((gt_ring_edges_kernel<float, OBJ, SELF>), dim3(static_cast<unsigned>(nctt), ny),
                         dim3(kThreads), 0, s, a, w_prev, w_next, w_self, n_rows, cs.n4 * 4, cs.tail);
  }, Ints<0, 1>{objective}, Bool{w_self != nullptr});
  return check_launch(nm);
}

}  // extern "C"
