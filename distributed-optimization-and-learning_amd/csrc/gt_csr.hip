// gt_csr.hip — one gradient-tracking round (DIGing / NEXT) on the agent-major
// bank with any sparse W in one HBM pass: dol_gt_csr_f32, the sibling of
// dol_gt_ring_f32 (gt_ring.hip, rings only) and of dol_gt_csr_pm_f32
// (pmajor.hip, at most 4096 agents).  Its own translation unit, so csr.o,
// gt_ring.o and their pinned kernels stay as they are.
//
// Layout as csr.hip: agent i's vector is row i of a row-major fp32 matrix.  Two
// row matrices, the parameters X and the trackers S, are gathered through ONE
// read of rowptr / col / val per row; the centre rows x_i, s_i and the target
// row t_i ride along.  For every row i and column c, all fp32, each operation
// rounded once (-ffp-contract=off):
//   ax = sum_e val[e] * x[col[e]]      (+0 start, ascending e: fmac())     as = the same over s
// and then gt_finish (dol_launch.h) with d = self_w[i], the lane that
// dol_gt_csr_pm_f32 and dol_gt_ring_f32 run too: the same bits as the first on
// the same CSR and as the second on a ring's CSR.  The Epi hook of
// csr_xcd_kernel / csr_mix_kernel cannot say this: an epilogue sees one mixed
// value, this round needs two mixes through one index and the centre rows of
// both (gt_ring.hip's header, for the ring).
//
// Policies: the gathered rows and the centre rows load with the default policy
// (a centre row is some other row's neighbour); the target row is read once and
// loads nontemporal; both stores are nontemporal.
//
//
// Tile width of the XCD-pinned form.  csr_xcd_kernel pins a 512-B column tile
// to one XCD so its slab (n x 512 B, 4 MiB at 8192 agents) lives in that XCD's
// 4 MiB L2.  This round has two slabs, 8 MiB at 8192 agents, so 512-B tiles
// were measured against 256-B ones (2 x 2 MiB): both instantiations in one
// build behind a per-call switch, alternating in one process, random 4-regular
// graph with Metropolis weights, P = 2^20, one box, medians of 7 windows of 10
// calls, least squares / logistic in ms (profiles/gt_csr_tile_width.jsonl):
//   agents  ld            512 B            256 B            dgd_csr + momentum, the same bytes
//   1024    2^20          5.96 / 6.05      5.94 / 6.01      4.51
//   1024    2^20 + 2048   5.09 / 5.21      5.35 / 5.58      3.89
//   8192    2^20 + 2048   44.48 / 44.75    47.56 / 47.87    31.51
// 512 B wins by 5-7 % on padded rows at both sizes and ties (0.4 % behind) on
// ld = 2^20; one width stays and the switch is gone.  The counters
// (tools/gt_counters.py, profiles/gt_csr_counters.json; FETCH_SIZE x 2
// against 3 N P 4) read 1.78 x the algorithmic bytes at 1024 agents and 2.48 x
// at 8192, written 1.000 x: gather re-reads do leave L2, most of them at 8192
// agents, yet halving the footprint bought no time there, so they are served
// by the Infinity Cache and the distance to dgd_csr (1.3-1.4 x at the same
// algorithmic bytes) has another part: per row and f4 column the round issues
// 11 loads (8 gathered, 2 centre, 1 target) where the DGD round issues 6.  Why
// a third of the re-reads miss at 1024 agents (1 MiB of slabs per tile) was
// not found.  Not measured:
// other rows-per-block counts (csr.hip's PASSES finding is taken over), 384-B
// tiles (they lost on the mix), an LDS-staged gather.
// Degree-4 fast path: all indices, then all 16 neighbour f4s of both matrices
// and the 6 centre / target f4s in flight per thread: 112-122 VGPRs, no scratch,
// 4 waves per SIMD.
#include "dol_launch.h"

namespace {
constexpr int kThreads = 256;  // 4 waves of 64
constexpr int kGtCsrRows = 16;  // rows per block of gt_csr_kernel (csr.hip's RPB)
constexpr int kGtCsrMinXcdRows = 512;  // the XCD-pinned form from this many rows (csr.hip's rule)

struct GtCsr {
  const float* X; int64_t ldx;
  const float* S; int64_t lds;
  float* XO; int64_t ldxo;
  float* SO; int64_t ldso;
  const float* T; int64_t ldt;
  float neg_lr;
};
// (rowptr, col, val and the self weights are kernel arguments of their own,
// const __restrict__, as in csr.hip and gt_ring.hip)

// ----------------------------------------------------------------------------
// 4 KiB column tiles (V = f4: 256 lanes x 16 B) or 1 KiB of scalar columns (V =
// float: the P % 4 tail, or every column when a row base is not 16-B aligned),
// kGtCsrRows rows per block, row group fastest as csr_mix_kernel: small graphs,
// and the f4 columns the pinned tiles leave over.  c_off: the first element
// column of this launch.
// ----------------------------------------------------------------------------
template <typename V, int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_csr_kernel(GtCsr a, int n_rows, int64_t c_off, int64_t ncols_v,
                                                          int64_t n_row_groups, const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col,
                                                          const float* __restrict__ val,
                                                          const float* __restrict__ wself) {
  constexpr int VW = Vec<V>::W;
  const int64_t b = blockIdx.x;
  const int rg = static_cast<int>(b % n_row_groups);
  const int64_t c = (b / n_row_groups) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  const int r0 = rg * kGtCsrRows;
  const int r1 = min(r0 + kGtCsrRows, n_rows);
  const int64_t cf = c_off + c * VW;  // element column
  const float* xb = a.X + cf;
  const float* sb = a.S + cf;
  auto xat = [&](int64_t r) { return *reinterpret_cast<const V*>(xb + r * a.ldx); };
  auto sat = [&](int64_t r) { return *reinterpret_cast<const V*>(sb + r * a.lds); };
  for (int r = r0; r < r1; ++r) {
    const V t = ldv<V, sizeof(V) == 16>(reinterpret_cast<const V*>(a.T + int64_t(r) * a.ldt + cf));
    const V xc = xat(r), sc = sat(r);
    const float ws = SELF ? wself[r] : 0.0f;
    const int e0 = rowptr[r];
    const int e1 = rowptr[r + 1];
    V ax = vzero(V{}), as = vzero(V{});
    int e = e0;
    for (; e + 4 <= e1; e += 4) {
      const int64_t c0 = col[e], c1 = col[e + 1], c2 = col[e + 2], c3 = col[e + 3];
      const V x0 = xat(c0), x1 = xat(c1), x2 = xat(c2), x3 = xat(c3);
      const V s0 = sat(c0), s1 = sat(c1), s2 = sat(c2), s3 = sat(c3);
      const float v0 = val[e], v1 = val[e + 1], v2 = val[e + 2], v3 = val[e + 3];
      ax = fmac(ax, v0, x0);
      as = fmac(as, v0, s0);
      ax = fmac(ax, v1, x1);
      as = fmac(as, v1, s1);
      ax = fmac(ax, v2, x2);
      as = fmac(as, v2, s2);
      ax = fmac(ax, v3, x3);
      as = fmac(as, v3, s3);
    }
    for (; e < e1; ++e) {
      const int64_t cj = col[e];
      const float v = val[e];
      ax = fmac(ax, v, xat(cj));
      as = fmac(as, v, sat(cj));
    }
    V xo, so;
    gt_finish<OBJ>(ax, as, xc, sc, t, ws, SELF, a.neg_lr, xo, so);
    __builtin_nontemporal_store(xo, reinterpret_cast<V*>(a.XO + int64_t(r) * a.ldxo + cf));
    __builtin_nontemporal_store(so, reinterpret_cast<V*>(a.SO + int64_t(r) * a.ldso + cf));
  }
}

// ----------------------------------------------------------------------------
// XCD-pinned form for large graphs with non-local neighbours, csr_xcd_kernel's
// sibling: a column tile is W f4 wide and every block of that tile has the same
// blockIdx % 8, so the tile's slabs of X and of S (n rows x 16 W bytes each)
// are fetched once into ONE XCD's L2 and the deg re-reads of each row hit
// there.  Placement is a speed assumption only: any other block -> XCD mapping
// gives the same results.  One block = (256 / W) x PASSES rows of the tile.
// Degree-4 rows (random-regular) gather every pass's indices, then every
// neighbour row of both matrices, then the centre and target rows, before any
// arithmetic; other degrees walk their lists 4 at a time.  Rows past the end
// of a ragged block read row n - 1's lists and rows (valid loads) and store
// nothing.
// ----------------------------------------------------------------------------
template <int W, int PASSES, int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_csr_xcd_kernel(GtCsr a, int n_rows, uint32_t nrb, uint32_t ntiles,
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
  const f4* tb = reinterpret_cast<const f4*>(a.T) + c;
  const int64_t ldxv = a.ldx / 4, ldsv = a.lds / 4, ldtv = a.ldt / 4;
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
  // the centre rows, the target row and the self weight of every pass: issued
  // ahead of the gathers on either path (clamped rows: valid loads)
  f4 xc[PASSES], sc[PASSES], tv[PASSES];
  float ws[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    xc[p] = xb[int64_t(rc[p]) * ldxv];
    sc[p] = sb[int64_t(rc[p]) * ldsv];
    tv[p] = __builtin_nontemporal_load(tb + int64_t(rc[p]) * ldtv);
    ws[p] = SELF ? wself[rc[p]] : 0.0f;
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
        f4 xo, so;
        gt_finish<OBJ>(ax, as, xc[p], sc[p], tv[p], ws[p], SELF, a.neg_lr, xo, so);
        __builtin_nontemporal_store(xo, reinterpret_cast<f4*>(a.XO + int64_t(rr[p]) * a.ldxo) + c);
        __builtin_nontemporal_store(so, reinterpret_cast<f4*>(a.SO + int64_t(rr[p]) * a.ldso) + c);
      }
    }
    return;
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int r = rr[p];
    if (r < n_rows) {
      f4 ax = f4{0.f, 0.f, 0.f, 0.f}, as = f4{0.f, 0.f, 0.f, 0.f};
      int e = e0[p];
      for (; e + 4 <= e1[p]; e += 4) {
        const int64_t c0 = col[e], c1 = col[e + 1], c2 = col[e + 2], c3 = col[e + 3];
        const f4 x0 = xb[c0 * ldxv], x1 = xb[c1 * ldxv], x2 = xb[c2 * ldxv], x3 = xb[c3 * ldxv];
        const f4 s0 = sb[c0 * ldsv], s1 = sb[c1 * ldsv], s2 = sb[c2 * ldsv], s3 = sb[c3 * ldsv];
        const float v0 = val[e], v1 = val[e + 1], v2 = val[e + 2], v3 = val[e + 3];
        ax = fmac(ax, v0, x0);
        as = fmac(as, v0, s0);
        ax = fmac(ax, v1, x1);
        as = fmac(as, v1, s1);
        ax = fmac(ax, v2, x2);
        as = fmac(as, v2, s2);
        ax = fmac(ax, v3, x3);
        as = fmac(as, v3, s3);
      }
      for (; e < e1[p]; ++e) {
        const int64_t cj = col[e];
        const float v = val[e];
        ax = fmac(ax, v, xb[cj * ldxv]);
        as = fmac(as, v, sb[cj * ldsv]);
      }
      f4 xo, so;
      gt_finish<OBJ>(ax, as, xc[p], sc[p], tv[p], ws[p], SELF, a.neg_lr, xo, so);
      __builtin_nontemporal_store(xo, reinterpret_cast<f4*>(a.XO + int64_t(r) * a.ldxo) + c);
      __builtin_nontemporal_store(so, reinterpret_cast<f4*>(a.SO + int64_t(r) * a.ldso) + c);
    }
  }
}

template <typename V, int OBJ, bool SELF>
void launch_gt_csr(const GtCsr& a, int n_rows, int64_t c_off, int64_t ncols_v, const int32_t* rowptr,
                   const int32_t* col, const float* val, const float* wself, hipStream_t s) {
  const int64_t n_rg = cdiv(n_rows, kGtCsrRows);
  hipLaunchKernelGGL((gt_csr_kernel<V, OBJ, SELF>), dim3(static_cast<unsigned>(cdiv(ncols_v, kThreads) * n_rg)),
                     dim3(kThreads), 0, s, a, n_rows, c_off, ncols_v, n_rg, rowptr, col, val, wself);
}

}  // namespace

extern "C" {

int dol_gt_csr_f32(const float* X, int64_t ldx, const float* S, int64_t lds, float* XO, int64_t ldxo, float* SO,
                   int64_t ldso, int32_t n, int64_t P, const int32_t* rowptr, const int32_t* col, const float* val,
                   const float* self_w, const float* target, int64_t ldt, int32_t objective, float lr,
                   hipStream_t s) {
  const char* nm = "dol_gt_csr_f32";
  const GtRows m{X, ldx, S, lds, XO, ldxo, SO, ldso, target, ldt};
  DOL_CHECKED(m.check(nm, n, P, !rowptr || !col || !val));
  if (const int rc = GtRows::objective_ok(nm, objective)) return rc;
  const ColSplit cs = split_cols(P, m.vec_ok());
  constexpr int XW = 32, XPASSES = 2;  // XCD-pinned tiles: 512 B of a row, 16 rows per block
  const int64_t n_rg = cdiv(n, kGtCsrRows);
  if (mul_sat(cdiv(cs.n4, kThreads), n_rg) > kMaxBlocks || mul_sat(cdiv(cs.tail, kThreads), n_rg) > kMaxBlocks)
    return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const bool use_xcd = cs.n4 >= XW && n >= kGtCsrMinXcdRows;
  const int64_t nt = use_xcd ? cs.n4 / XW : 0;
  const int64_t nrb = cdiv(n, (kThreads / XW) * XPASSES);
  if (cdiv(nt, 8) * 8 * nrb > kMaxBlocks * 8) return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const int64_t done4 = nt * XW;
  const GtCsr a{X, ldx, S, lds, XO, ldxo, SO, ldso, target, ldt, -lr};
  dispatch([&](auto obj, auto self) {
    constexpr int OBJ = decltype(obj)::value;
    constexpr bool SELF = decltype(self)::value;
    if (nt > 0)
      hipLaunchKernelGGL((gt_csr_xcd_kernel<XW, XPASSES, OBJ, SELF>),
                         dim3(static_cast<unsigned>(cdiv(nt, 8) * 8 * nrb)), dim3(kThreads), 0, s, a, n,
                         static_cast<uint32_t>(nrb), static_cast<uint32_t>(nt), rowptr, col, val, self_w);
    if (cs.n4 > done4)
      launch_gt_csr<f4, OBJ, SELF>(a, n, done4 * 4, cs.n4 - done4, rowptr, col, val, self_w, s);
    if (cs.tail > 0) launch_gt_csr<float, OBJ, SELF>(a, n, cs.n4 * 4, cs.tail, rowptr, col, val, self_w, s);
  }, Ints<0, 1>{objective}, Bool{self_w != nullptr});
  return check_launch(nm);
}

}  // extern "C"
