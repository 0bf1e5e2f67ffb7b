// gt_csr.hip — one gradient-tracking round on the agent-major bank with any
// sparse weight matrix in one HBM pass, in two forms that share every kernel:
//   dol_gt_csr_f32       DIGing / NEXT with a doubly stochastic W, the sibling
//                        of dol_gt_ring_f32 (gt_ring.hip, rings only) and of
//                        dol_gt_csr_pm_f32 (pmajor.hip, at most 4096 agents);
//   dol_gt_push_csr_f32  push-sum gradient tracking (ADD-OPT, Xi-Xin-Khan 2018;
//                        Push-DIGing in combine-then-adapt form) with a
//                        column-stochastic C, for weights that are not doubly
//                        stochastic.
//
// Layout as csr.hip: agent i's vector is row i of a row-major fp32 matrix.  Two
// row matrices, the parameters X (the push-sum numerators U of the push-sum
// round) and the trackers S, are gathered through ONE read of rowptr / col /
// val per row; the centre rows x_i, s_i and the target row t_i ride along.  For
// every row i and column c, all fp32, each operation rounded once
// (-ffp-contract=off):
//   ax = sum_e val[e] * x[col[e]]      (+0 start, ascending e: fmac())     as = the same over s
// and then gt_finish (dol_launch.h) with d = self_w[i], the lane that
// dol_gt_csr_pm_f32 and dol_gt_ring_f32 run too: the same bits as the first on
// the same CSR and as the second on a ring's CSR.  The Epi hook of
// csr_xcd_kernel / csr_mix_kernel cannot say this: an epilogue sees one mixed
// value, this round needs two mixes through one index and the centre rows of
// both (gt_ring.hip's header, for the ring).
//
// The push-sum round: C = C_off + diag(self_w), C_off the CSR whose row i lists
// i's in-neighbours.  Beside the two mixes above (x = u),
//   av = sum_e val[e] * v[col[e]]      (the same rounding, on the n-vector v)
//   av = fl(av + fl(d_i v_i)) with self weights;   v'_i = av
// and then gt_push_finish (dol_launch.h) with d = self_w[i], v = v[i], av =
// v'[i]: the gradients are taken at z = u / v and z' = u' / av, two correctly
// rounded divisions per coordinate.  z is not stored (it is U / v), so the
// round moves the five streams of dol_gt_csr_f32 plus 2 n floats.
// How v' is produced: gt_push_v_kernel (n threads) runs first in the same call
// and writes v_out; the main kernels, ordered after it on the stream, read
// v[i] and v_out[i] as two per-row scalars.  The degree-4 fast path's register
// budget is the reason: the mix of v inside the main kernels would add a third
// gather to it.
//
// One kernel body for both rounds.  gt_csr_kernel and gt_csr_xcd_kernel take
// the round as their first template parameter, a tag (GtPlain, GtPushSum) that
// names the per-row scalars (Row, load) and the lane (finish); geometry,
// policies and clamped ragged rows are the same text for both.  Two rules keep
// the emitted code what it was when each round had kernels of its own:
//   * the tag stays stateless: a type, never an object passed to the kernel;
//   * v and vnew stay `const float* __restrict__` kernel parameters (two null
//     pointers that are never read in the plain round).
// Carried as __restrict__ members of a policy object passed by value they lose
// their alias information: the f4 small-n push-sum kernels went from 78 / 80
// VGPRs to 82 / 84 and from 6 waves per SIMD to 5, the scalar ones from 40 to
// 42 (the pinned kernels were unaffected).
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
// tiles (they lost on the mix), an LDS-staged gather.  (All of the above is the
// plain round's; not measured again for the push-sum round, nor when the two
// rounds were given one body.)
// Degree-4 fast path: all indices, then all 16 neighbour f4s of both matrices
// and the 6 centre / target f4s in flight per thread: 112-122 VGPRs, no scratch,
// 4 waves per SIMD.
//
// Resource usage, from the compiler's kernel-resource-usage remarks (gfx950,
// -O3; occupancy in waves per SIMD; no instantiation uses scratch or LDS):
//   kernel                                  VGPRs: LS / LS+self / logistic / logistic+self   scratch   occupancy
//   gt_csr_xcd_kernel<GtPlain, 32, 2>       112 / 122 / 115 / 119                            0         4
//   gt_csr_kernel<GtPlain, f4>              78 / 78 / 80 / 80                                0         6
//   gt_csr_kernel<GtPlain, float>           40 / 40 / 40 / 40                                0         8
//   gt_csr_xcd_kernel<GtPushSum, 32, 2>     118 / 119 / 126 / 122                            0         4
//   gt_csr_kernel<GtPushSum, f4>            78 / 78 / 80 / 80                                0         6
//   gt_csr_kernel<GtPushSum, float>         40 / 40 / 40 / 40                                0         8
//   gt_push_v_kernel                        12 (with and without self weights)               0         8
// The pinned push-sum kernel keeps the plain one's 4 waves per SIMD (128 VGPRs):
// the two per-row scalars and the divisions' temporaries fit beside its 112-122.
#include "dol_launch.h"

namespace {
constexpr int kThreads = 256;  // 4 waves of 64
constexpr int kRows = 16;  // rows per block of gt_csr_kernel (csr.hip's RPB)
constexpr int kMinXcdRows = 512;  // the XCD-pinned form from this many rows (csr.hip's rule)

struct GtCsr {
  const float* X; int64_t ldx;
  const float* S; int64_t lds;
  float* XO; int64_t ldxo;
  float* SO; int64_t ldso;
  const float* T; int64_t ldt;
  float neg_lr;
};
// (rowptr, col, val, the self weights and the two push-sum weight vectors are
// kernel arguments of their own, const __restrict__, as in csr.hip and
// gt_ring.hip)

// The round tags.  Row: what a row carries beside its self weight; load(): read
// it at row r; finish(): the lane of dol_launch.h.
struct GtPlain {
  struct Row {};
  static __device__ __forceinline__ Row load(const float*, const float*, int64_t) { return {}; }
  template <int OBJ, bool SELF, typename V>
  static __device__ __forceinline__ void finish(V ax, V as, V x, V s, V t, float d, float neg_lr, Row, V& xo, V& so) {
    gt_finish<OBJ>(ax, as, x, s, t, d, SELF, neg_lr, xo, so);
  }
};
struct GtPushSum {
  struct Row { float v, av; };  // the agent's push-sum weight before the round and after it
  static __device__ __forceinline__ Row load(const float* __restrict__ v, const float* __restrict__ vnew, int64_t r) {
    return {v[r], vnew[r]};
  }
  template <int OBJ, bool SELF, typename V>
  static __device__ __forceinline__ void finish(V au, V as, V u, V s, V t, float d, float neg_lr, Row w, V& uo, V& so) {
    gt_push_finish<OBJ>(au, as, u, s, t, d, SELF, neg_lr, w.v, w.av, uo, so);
  }
};

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
// 4 KiB column tiles (V = f4: 256 lanes x 16 B) or 1 KiB of scalar columns (V =
// float: the P % 4 tail, or every column when a row base is not 16-B aligned),
// kRows rows per block, row group fastest as csr_mix_kernel: small graphs, and
// the f4 columns the pinned tiles leave over.  c_off: the first element column
// of this launch.
// ----------------------------------------------------------------------------
template <class R, typename V, int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_csr_kernel(GtCsr a, int n_rows, int64_t c_off, int64_t ncols_v,
                                                          int64_t n_row_groups, const int32_t* __restrict__ rowptr,
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
  const int r0 = rg * kRows;
  const int r1 = min(r0 + kRows, n_rows);
  const int64_t cf = c_off + c * VW;  // element column
  const float* xb = a.X + cf;
  const float* sb = a.S + cf;
  auto xat = [&](int64_t r) { return *reinterpret_cast<const V*>(xb + r * a.ldx); };
  auto sat = [&](int64_t r) { return *reinterpret_cast<const V*>(sb + r * a.lds); };
  for (int r = r0; r < r1; ++r) {
    const V t = ldv<V, sizeof(V) == 16>(reinterpret_cast<const V*>(a.T + int64_t(r) * a.ldt + cf));
    const V xc = xat(r), sc = sat(r);
    const float ws = SELF ? wself[r] : 0.0f;
    const typename R::Row row = R::load(v, vnew, r);
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
    R::template finish<OBJ, SELF>(ax, as, xc, sc, t, ws, a.neg_lr, row, xo, so);
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
// of a ragged block read row n - 1's lists, rows and push-sum weights (valid
// loads) and store nothing.
// ----------------------------------------------------------------------------
template <class R, int W, int PASSES, int OBJ, bool SELF>
__global__ __launch_bounds__(kThreads) void gt_csr_xcd_kernel(GtCsr a, int n_rows, uint32_t nrb, uint32_t ntiles,
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
  // the centre rows, the target row, the self weight and the round's own row
  // scalars of every pass: issued ahead of the gathers on either path (clamped
  // rows: valid loads)
  f4 xc[PASSES], sc[PASSES], tv[PASSES];
  float ws[PASSES];
  typename R::Row row[PASSES];
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    xc[p] = xb[int64_t(rc[p]) * ldxv];
    sc[p] = sb[int64_t(rc[p]) * ldsv];
    tv[p] = __builtin_nontemporal_load(tb + int64_t(rc[p]) * ldtv);
    ws[p] = SELF ? wself[rc[p]] : 0.0f;
    row[p] = R::load(v, vnew, rc[p]);
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
        R::template finish<OBJ, SELF>(ax, as, xc[p], sc[p], tv[p], ws[p], a.neg_lr, row[p], xo, so);
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
      f4 xo, so;
      R::template finish<OBJ, SELF>(ax, as, xc[p], sc[p], tv[p], ws[p], a.neg_lr, row[p], xo, so);
      __builtin_nontemporal_store(xo, reinterpret_cast<f4*>(a.XO + int64_t(r) * a.ldxo) + c);
      __builtin_nontemporal_store(so, reinterpret_cast<f4*>(a.SO + int64_t(r) * a.ldso) + c);
    }
  }
}

template <class R, typename V, int OBJ, bool SELF>
void launch_gt_csr(const GtCsr& a, int n_rows, int64_t c_off, int64_t ncols_v, const int32_t* rowptr,
                   const int32_t* col, const float* val, const float* wself, const float* v, const float* vnew,
                   hipStream_t s) {
  const int64_t n_rg = cdiv(n_rows, kRows);
  hipLaunchKernelGGL((gt_csr_kernel<R, V, OBJ, SELF>), dim3(static_cast<unsigned>(cdiv(ncols_v, kThreads) * n_rg)),
                     dim3(kThreads), 0, s, a, n_rows, c_off, ncols_v, n_rg, rowptr, col, val, wself, v, vnew);
}

// What both entry points do once their own argument rules have passed: the
// column split, the launch-size rules, the XCD decision and the launches.
// first(self): the round's own launch ahead of the main kernels (v' = C v).
template <class R, class First>
int gt_csr_round(const char* nm, const GtRows& m, int32_t n, int64_t P, const int32_t* rowptr, const int32_t* col,
                 const float* val, const float* self_w, int32_t objective, float lr, const float* v,
                 const float* vnew, hipStream_t s, First first) {
  const ColSplit cs = split_cols(P, m.vec_ok());
  constexpr int XW = 32, XPASSES = 2;  // XCD-pinned tiles: 512 B of a row, 16 rows per block
  const int64_t n_rg = cdiv(n, kRows);
  if (mul_sat(cdiv(cs.n4, kThreads), n_rg) > kMaxBlocks || mul_sat(cdiv(cs.tail, kThreads), n_rg) > kMaxBlocks)
    return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const bool use_xcd = cs.n4 >= XW && n >= kMinXcdRows;
  const int64_t nt = use_xcd ? cs.n4 / XW : 0;
  const int64_t nrb = cdiv(n, (kThreads / XW) * XPASSES);
  if (cdiv(nt, 8) * 8 * nrb > kMaxBlocks * 8) return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  const int64_t done4 = nt * XW;
  const GtCsr a{m.X, m.ldx, m.S, m.lds, m.XO, m.ldxo, m.SO, m.ldso, m.T, m.ldt, -lr};
  dispatch([&](auto obj, auto self) {
    constexpr int OBJ = decltype(obj)::value;
    constexpr bool SELF = decltype(self)::value;
    first(self);
    if (nt > 0)
      hipLaunchKernelGGL((gt_csr_xcd_kernel<R, XW, XPASSES, OBJ, SELF>),
                         dim3(static_cast<unsigned>(cdiv(nt, 8) * 8 * nrb)), dim3(kThreads), 0, s, a, n,
                         static_cast<uint32_t>(nrb), static_cast<uint32_t>(nt), rowptr, col, val, self_w, v, vnew);
    if (cs.n4 > done4)
      launch_gt_csr<R, f4, OBJ, SELF>(a, n, done4 * 4, cs.n4 - done4, rowptr, col, val, self_w, v, vnew, s);
    if (cs.tail > 0)
      launch_gt_csr<R, float, OBJ, SELF>(a, n, cs.n4 * 4, cs.tail, rowptr, col, val, self_w, v, vnew, s);
  }, Ints<0, 1>{objective}, Bool{self_w != nullptr});
  return check_launch(nm);
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
  return gt_csr_round<GtPlain>(nm, m, n, P, rowptr, col, val, self_w, objective, lr, nullptr, nullptr, s, [](auto) {});
}

int dol_gt_push_csr_f32(const float* U, int64_t ldu, const float* S, int64_t lds, float* UO, int64_t lduo, float* SO,
                        int64_t ldso, int32_t n, int64_t P, const int32_t* rowptr, const int32_t* col,
                        const float* val, const float* self_w, const float* target, int64_t ldt, int32_t objective,
                        float lr, const float* v, float* v_out, hipStream_t s) {
  const char* nm = "dol_gt_push_csr_f32";
  const GtRows m{U, ldu, S, lds, UO, lduo, SO, ldso, target, ldt};
  DOL_CHECKED(m.check(nm, n, P, !rowptr || !col || !val || !v || !v_out));
  if (const int rc = GtRows::objective_ok(nm, objective)) return rc;
  if (v == v_out) return fail(DOL_EINVAL, "%s: v and v_out alias (every v' reads its neighbours' v)", nm);
  // v' = C v first: the main kernels read it, ordered after it on the stream
  return gt_csr_round<GtPushSum>(nm, m, n, P, rowptr, col, val, self_w, objective, lr, v, v_out, s, [&](auto self) {
    hipLaunchKernelGGL((gt_push_v_kernel<decltype(self)::value>), dim3(static_cast<unsigned>(cdiv(n, kThreads))),
                       dim3(kThreads), 0, s, n, rowptr, col, val, self_w, v, v_out);
  });
}

}  // extern "C"
