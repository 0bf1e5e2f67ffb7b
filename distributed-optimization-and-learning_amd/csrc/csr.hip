// csr.hip — the generic sparse (CSR) mix on the agent-major bank and its
// fused DGD and EXTRA rounds (EXTRA also with the gradient fed as a row matrix):
// 4 KiB column tiles, or XCD-pinned 512 B tiles from 512 rows.
//
// Dropped launch variant (8192 x 2^20; the default's bits; code last present at 1a824fc):
//   DOL_CSR_PASSES=1|4: csr_xcd_kernel with 8 / 32 rows per block instead of 16: 512-B tiles 17.94 ms
//     with 1 pass vs 17.01 with 2; 256-B tiles 18.99 with 4 vs 18.52 (profiles/r01_membench6_csr.txt).
// The switch that stays: DOL_CSR_MODE (both kernels it selects are live under the automatic rule).
#include "dol_launch.h"

namespace {
constexpr int kThreads = 256;            // 4 waves of 64

// ----------------------------------------------------------------------------
// Generic CSR mix.  Blocks are ordered row-group fastest so that all rows of
// one column tile are in flight together: a neighbour row segment fetched
// from HBM by one workgroup is re-read from L2 / Infinity Cache by the others.
// ----------------------------------------------------------------------------
template <typename V, int RPB, class Epi = NoEpi>
__global__ __launch_bounds__(kThreads) void csr_mix_kernel(
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int n_rows,
    int64_t c_off, int64_t ncols_v, int64_t n_row_groups, const int32_t* __restrict__ rowptr,
    const int32_t* __restrict__ col, const float* __restrict__ val, Epi epi) {
  const int64_t b = blockIdx.x;
  const int rg = static_cast<int>(b % n_row_groups);
  const int64_t ct = b / n_row_groups;
  const int64_t c = ct * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  const int r0 = rg * RPB;
  const int r1 = min(r0 + RPB, n_rows);
  const V* xb = reinterpret_cast<const V*>(X + c_off) + c;
  const int64_t cf = c_off + c * Vec<V>::W;
  for (int r = r0; r < r1; ++r) {
    const auto es = epi.template load<V>(r, cf);
    const int e0 = rowptr[r];
    const int e1 = rowptr[r + 1];
    V acc = vzero(V{});
    int e = e0;
    for (; e + 4 <= e1; e += 4) {
      const V x0 = xb[int64_t(col[e + 0]) * (ldx / Vec<V>::W)];
      const V x1 = xb[int64_t(col[e + 1]) * (ldx / Vec<V>::W)];
      const V x2 = xb[int64_t(col[e + 2]) * (ldx / Vec<V>::W)];
      const V x3 = xb[int64_t(col[e + 3]) * (ldx / Vec<V>::W)];
      acc = fmac(acc, val[e + 0], x0);
      acc = fmac(acc, val[e + 1], x1);
      acc = fmac(acc, val[e + 2], x2);
      acc = fmac(acc, val[e + 3], x3);
    }
    for (; e < e1; ++e) acc = fmac(acc, val[e], xb[int64_t(col[e]) * (ldx / Vec<V>::W)]);
    acc = epi.apply(acc, es, r, cf);
    __builtin_nontemporal_store(acc, reinterpret_cast<V*>(Y + int64_t(r) * ldy + c_off) + c);
  }
}

// XCD-pinned CSR mix for large graphs with non-local neighbours (random-
// regular, ER as sparse): a column tile is W f4 wide (512 B of a row), and
// every block of that tile has the same blockIdx % 8 — the dispatcher deals
// blocks round-robin over the 8 XCDs, so the tile's whole X slab (n rows x
// 512 B, 4 MiB at 8192 agents) is fetched once into ONE XCD's L2 and the deg
// re-reads of each row hit there.  Placement is a speed assumption only: any
// other block->XCD mapping gives the same results.  Measured at 8192 x 2^20,
// d = 4 (tools/membench6.hip): 4.04 TB/s vs 3.0 with 4 KiB tiles whose 32 MiB
// slabs re-read through the Infinity Cache.  Degree-4 rows (random-regular)
// gather all passes' indices before any neighbour load (16.68 vs 16.80 ms).
// A persistent variant (a fixed grid per XCD walking the tiles in step, so
// only one slab is live in L2) ran 25-46 ms: latency-bound, dropped.  A
// persistent sweep (each workgroup holding 64 rows' partial sums in LDS, every
// row group's neighbour lists merged into one j-ascending list, so all readers
// of a line touch it together) was bit-exact but ran 27 ms with either tile
// order (profiles/r01d_csr_sweep_kernel.txt), dropped.  Tile
// widths (same box, 8192 x 2^20): 512 B 16.7 ms, 384 B (240-thread blocks)
// 22.6 ms, 256 B 18.2 ms.
template <int W, int PASSES, class Epi = NoEpi>
__global__ __launch_bounds__(kThreads) void csr_xcd_kernel(
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int n_rows,
    uint32_t nrb, uint32_t ntiles, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
    const float* __restrict__ val, Epi epi) {
  constexpr int ROWS = kThreads / W;
  constexpr int RB = ROWS * PASSES;
  const uint32_t b = blockIdx.x;
  const uint32_t xcd = b & 7u, local = b >> 3;
  const uint32_t tloc = local / nrb, rb = local % nrb;
  const uint32_t ct = tloc * 8 + xcd;
  if (ct >= ntiles) return;
  const int lane_c = threadIdx.x % W, lane_r = threadIdx.x / W;
  const int64_t c = int64_t(ct) * W + lane_c;  // f4 column
  const f4* xb = reinterpret_cast<const f4*>(X) + c;
  const int64_t ldv = ldx / 4;
  // every pass's row extent first, then (degree-4 rows, the random-regular
  // case) every pass's neighbour indices, then all neighbour loads: three
  // dependent round trips per workgroup instead of three per pass
  int rr[PASSES], e0[PASSES], e1[PASSES];
  bool four = true;
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    rr[p] = int(rb) * RB + p * ROWS + lane_r;
    const int rc = rr[p] < n_rows ? rr[p] : n_rows - 1;
    e0[p] = rowptr[rc];
    e1[p] = rowptr[rc + 1];
    four = four && (e1[p] - e0[p] == 4);
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
    f4 xs[PASSES][4];
#pragma unroll
    for (int p = 0; p < PASSES; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) xs[p][q] = xb[int64_t(cc[p][q]) * ldv];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      if (rr[p] < n_rows) {
        const auto es = epi.template load<f4>(rr[p], 4 * c);
        f4 acc = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = fmac(acc, vv[p][q], xs[p][q]);
        acc = epi.apply(acc, es, rr[p], 4 * c);
        __builtin_nontemporal_store(acc, reinterpret_cast<f4*>(Y + int64_t(rr[p]) * ldy) + c);
      }
    }
    return;
  }
#pragma unroll
  for (int p = 0; p < PASSES; ++p) {
    const int r = rr[p];
    if (r < n_rows) {
      const auto es = epi.template load<f4>(r, 4 * c);
      f4 acc = f4{0.f, 0.f, 0.f, 0.f};
      int e = e0[p];
      for (; e + 4 <= e1[p]; e += 4) {
        const f4 x0 = xb[int64_t(col[e]) * ldv], x1 = xb[int64_t(col[e + 1]) * ldv];
        const f4 x2 = xb[int64_t(col[e + 2]) * ldv], x3 = xb[int64_t(col[e + 3]) * ldv];
        acc = fmac(acc, val[e], x0);
        acc = fmac(acc, val[e + 1], x1);
        acc = fmac(acc, val[e + 2], x2);
        acc = fmac(acc, val[e + 3], x3);
      }
      for (; e < e1[p]; ++e) acc = fmac(acc, val[e], xb[int64_t(col[e]) * ldv]);
      acc = epi.apply(acc, es, r, 4 * c);
      __builtin_nontemporal_store(acc, reinterpret_cast<f4*>(Y + int64_t(r) * ldy) + c);
    }
  }
}

template <typename V, int RPB, class Epi = NoEpi>
void launch_csr(const float* X, int64_t ldx, float* Y, int64_t ldy, int n_rows, int64_t c_off,
                int64_t ncols_v, const int32_t* rowptr, const int32_t* col, const float* val,
                hipStream_t s, const Epi& epi = Epi{}) {
  const int64_t n_col_tiles = cdiv(ncols_v, kThreads);
  const int64_t n_rg = cdiv(n_rows, RPB);
  hipLaunchKernelGGL((csr_mix_kernel<V, RPB, Epi>), dim3(static_cast<unsigned>(n_col_tiles * n_rg)), dim3(kThreads), 0,
                     s, X, ldx, Y, ldy, n_rows, c_off, ncols_v, n_rg, rowptr, col, val, epi);
}

// Shared bodies of the plain and epilogue (DGD) forms of the two sparse mixes.
template <class Epi>
int mix_csr_impl(const char* nm, const float* X, int64_t ldx, int32_t x_rows, float* Y, int64_t ldy,
                 int32_t n_rows, int64_t P, const int32_t* rowptr, const int32_t* col, const float* val,
                 const Epi& epi, bool epi_vec_ok, hipStream_t s) {
  DOL_CHECKED(check_rows(nm, n_rows < 0 || P < 0 || x_rows < 0, n_rows == 0 || P == 0,
                         !X || !Y || !rowptr || (!col && x_rows > 0) || (!val && x_rows > 0), ldx < P || ldy < P,
                         X == Y, kJacobiAlias));
  const bool vec_ok = row_vec_ok(X, ldx) && row_vec_ok(Y, ldy) && epi_vec_ok;
  const ColSplit cs = split_cols(P, vec_ok);
  constexpr int RPB = 16;
  constexpr int XW = 32, XPASSES = 2;  // XCD-pinned tiles: 512 B of a row, 16 rows per block
  // 0 = 4 KiB tiles, 1 = XCD-pinned (DOL_CSR_MODE; default: XCD-pinned from 512 rows).
  // The switch stays: both kernels it selects are live under the automatic rule.
  const int mode = env_int("DOL_CSR_MODE", -1);
  if (mul_sat(cdiv(cs.n4, kThreads), cdiv(n_rows, RPB)) > kMaxBlocks)
    return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
  int64_t done4 = 0;
  const bool use_xcd = cs.n4 >= XW && (mode == 1 || (mode < 0 && n_rows >= 512));
  if (use_xcd) {
    const int64_t nt = cs.n4 / XW;
    const int64_t nrb = cdiv(n_rows, (kThreads / XW) * XPASSES);
    const int64_t grid = cdiv(nt, 8) * 8 * nrb;
    if (grid > kMaxBlocks * 8) return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
    hipLaunchKernelGGL((csr_xcd_kernel<XW, XPASSES, Epi>), dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s, X,
                       ldx, Y, ldy, n_rows, static_cast<uint32_t>(nrb), static_cast<uint32_t>(nt), rowptr, col, val,
                       epi);
    done4 = nt * XW;
  }
  if (cs.n4 > done4)  // column offset through c_off so the epilogue sees absolute columns
    launch_csr<f4, RPB, Epi>(X, ldx, Y, ldy, n_rows, done4 * 4, cs.n4 - done4, rowptr, col, val, s, epi);
  if (cs.tail > 0)
    launch_csr<float, RPB, Epi>(X, ldx, Y, ldy, n_rows, cs.n4 * 4, cs.tail, rowptr, col, val, s, epi);
  return check_launch(nm);
}

}  // namespace

extern "C" {

int dol_mix_csr_f32(const float* X, int64_t ldx, int32_t x_rows, float* Y, int64_t ldy,
                    int32_t n_rows, int64_t P, const int32_t* rowptr, const int32_t* col,
                    const float* val, hipStream_t s) {
  DOL_DIMS_OK("dol_mix_csr_f32", ldx, ldy, P);
  return mix_csr_impl("dol_mix_csr_f32", X, ldx, x_rows, Y, ldy, n_rows, P, rowptr, col, val, NoEpi{}, true, s);
}

int dol_dgd_csr_f32(const float* X, int64_t ldx, int32_t x_rows, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                    const int32_t* rowptr, const int32_t* col, const float* val, const float* target, int64_t ldt,
                    float* mom, int64_t ldm, int32_t objective, int32_t local_steps, float lr, float momentum,
                    int first_step, hipStream_t s) {
  DOL_DIMS_OK("dol_dgd_csr_f32", ldx, ldy, P, ldt, ldm);
  const char* nm = "dol_dgd_csr_f32";
  const DgdArgs d{target, ldt, mom, ldm, objective, local_steps, lr, momentum, first_step};
  return with_dgd_epi(nm, d, n_rows <= 0 || P <= 0, P, [&](auto epi, bool evec) {
    return mix_csr_impl(nm, X, ldx, x_rows, Y, ldy, n_rows, P, rowptr, col, val, epi, evec, s);
  });
}

// the EXTRA round (ExtraEpi, dol_launch.h): W is square, so the centre of output row i is row i of X
int dol_extra_csr_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n, int64_t P, const int32_t* rowptr,
                      const int32_t* col, const float* val, const float* self_w, const float* target, int64_t ldt,
                      float* corr, int64_t ldc, int32_t objective, float lr, hipStream_t s) {
  DOL_DIMS_OK("dol_extra_csr_f32", ldx, ldy, P, ldt, ldc);
  const char* nm = "dol_extra_csr_f32";
  const ExtraArgs e{target, ldt, corr, ldc, self_w, objective, lr};
  return with_extra_epi<false>(nm, e, X, ldx, Y, n <= 0 || P <= 0, P, [&](auto epi, bool evec) {
    return mix_csr_impl(nm, X, ldx, n, Y, ldy, n, P, rowptr, col, val, epi, evec, s);
  });
}

// the same round with the gradient fed as the row matrix G where the target is read (ExtraEpi<kObjGradRow>);
// its gradient-tracking sibling dol_gt_grad_csr_f32 has kernels of its own (grad_rounds.hip)
int dol_extra_grad_csr_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n, int64_t P,
                           const int32_t* rowptr, const int32_t* col, const float* val, const float* self_w,
                           const float* G, int64_t ldg, float* corr, int64_t ldc, float lr, hipStream_t s) {
  DOL_DIMS_OK("dol_extra_grad_csr_f32", ldx, ldy, P, ldg, ldc);
  const char* nm = "dol_extra_grad_csr_f32";
  const ExtraArgs e{G, ldg, corr, ldc, self_w, kObjGradRow, lr};
  return with_extra_grad_epi<false>(nm, e, X, ldx, Y, n <= 0 || P <= 0, P, [&](auto epi, bool evec) {
    return mix_csr_impl(nm, X, ldx, n, Y, ldy, n, P, rowptr, col, val, epi, evec, s);
  });
}

}  // extern "C"
