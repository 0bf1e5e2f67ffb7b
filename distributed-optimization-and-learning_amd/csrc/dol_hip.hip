// dol_hip.hip — what the whole library shares: the error plumbing behind
// dol_last_error, the version, the bank's VMM allocator (host code only) and
// the calibration copy.  The kernels live by family: ring.hip, csr.hip,
// admm.hip, dense_mix.hip (this file was all of them once), pmajor.hip,
// csr_slab.hip, dense_split.hip, mlp_step.hip, graph_draw.hip; what they share
// is in dol_launch.h.
//
// Build (see csrc/Makefile):  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared
// -ffp-contract=off is load-bearing: the reference (torch CPU) rounds every
// product and every sum separately in the mixing / dual / prox arithmetic, so
// the only fused multiply-adds are the explicit __builtin_fmaf of the SGD
// parameter updates (ATen's vectorised add_(d, alpha=-lr) is an FMA).
// The switch that stays here: DOL_BANK_* (tested behaviour).
#include <stdarg.h>
#include <stdio.h>
#include <mutex>
#include <unordered_map>

#include "dol_launch.h"

// error plumbing (shared with the other translation units via dol_common.h)
namespace dol {
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    return fail(-static_cast<int>(e), "%s: launch failed: %s", what, hipGetErrorString(e));
  }
  g_err[0] = '\0';
  return DOL_OK;
}
}  // namespace dol

namespace {
constexpr int kThreads = 256;            // 4 waves of 64

// Calibration copy: each block streams one contiguous 16 KiB chunk (4 x f4
// per lane, nontemporal both ways) and exits — 6.26 TB/s on MI355X, the
// measured ceiling the mixing kernels are compared with (tools/membench.hip).
__global__ __launch_bounds__(kThreads) void copy_kernel(const f4* __restrict__ src, f4* __restrict__ dst,
                                                        int64_t n) {
  const int64_t base = int64_t(blockIdx.x) * kThreads * 4 + threadIdx.x;
  f4 v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (base + u * kThreads < n) v[u] = __builtin_nontemporal_load(src + base + u * kThreads);
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (base + u * kThreads < n) __builtin_nontemporal_store(v[u], dst + base + u * kThreads);
}

__global__ __launch_bounds__(kThreads) void copy_scalar_kernel(const float* __restrict__ src,
                                                               float* __restrict__ dst, int64_t n) {
  const int64_t stride = int64_t(gridDim.x) * kThreads;
  for (int64_t i = int64_t(blockIdx.x) * kThreads + threadIdx.x; i < n; i += stride) dst[i] = src[i];
}

}  // namespace

// ============================================================================
// C-ABI
// ============================================================================
extern "C" {

int dol_version(void) { return 100; }

const char* dol_last_error(void) { return g_err; }

struct BankBlock {
  hipMemGenericAllocationHandle_t handle;
  size_t size;    // the mapped (granularity-rounded) size: what unmap / address-free take
  int stage = 0;  // 0 mapped, 1 unmapped, 2 range freed (dol_bank_free resumes from here)
};
static std::mutex g_bank_mu;  // dol_bank_alloc's live blocks: VA -> physical handle + mapped size
static std::unordered_map<void*, BankBlock> g_bank_handles;
// Virtual address space retired by dol_bank_free (see there) -- counted, and
// capped: past the cap dol_bank_alloc refuses new blocks instead of reserving
// address space without bound.  Guarded by g_bank_mu.
static int64_t g_bank_retired = 0;
static int64_t g_bank_retired_blocks = 0;

int64_t dol_bank_retired_cap_bytes(void) {
  const int64_t gib = env_int("DOL_BANK_RETIRED_VA_CAP_GIB", 4096);  // 4 TiB: 128 retired 32 GiB matrices
  return gib > 0 ? gib << 30 : 0;
}

int64_t dol_bank_retired_bytes(void) {
  std::lock_guard<std::mutex> lk(g_bank_mu);
  return g_bank_retired;
}

int64_t dol_bank_retired_blocks(void) {
  std::lock_guard<std::mutex> lk(g_bank_mu);
  return g_bank_retired_blocks;
}

// A bank buffer as ONE physical allocation (hipMemCreate) mapped into a
// reserved VA range, instead of whatever hipMalloc's suballocator returns
// (tools/alloc_probe.hip measures the ring round on both).
int dol_bank_alloc(int64_t bytes, void** ptr, int64_t* mapped_bytes) {
  if (!ptr || !mapped_bytes || bytes <= 0 || bytes > 4 * dol::kMaxDim)
    return fail(DOL_EINVAL, "dol_bank_alloc: bad arguments");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fail(DOL_EINVAL, "dol_bank_alloc: no device");
  *ptr = nullptr;
  *mapped_bytes = 0;
  hipMemAllocationProp prop{};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = dev;
  size_t gran = 0;
  hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
  if (e != hipSuccess || gran == 0) return fail(-static_cast<int>(e ? e : hipErrorInvalidValue), "dol_bank_alloc: granularity: %s", hipGetErrorString(e));
  const size_t size = (static_cast<size_t>(bytes) + gran - 1) / gran * gran;
  if (!env_int("DOL_BANK_FREE_VA", 0)) {  // this block's range will be retired when freed: stay under the cap
    std::lock_guard<std::mutex> lk(g_bank_mu);
    int64_t live = 0;
    for (const auto& kv : g_bank_handles) live += static_cast<int64_t>(kv.second.size);
    const int64_t cap = dol_bank_retired_cap_bytes();
    if (g_bank_retired + live + static_cast<int64_t>(size) > cap)
      return fail(DOL_ECAP, "dol_bank_alloc: %zu bytes would take the retired + live mapped address space "
                  "(%lld + %lld bytes) past its cap of %lld bytes (DOL_BANK_RETIRED_VA_CAP_GIB); use torch's "
                  "allocator (DOL_BANK_ALLOC=torch)", size, static_cast<long long>(g_bank_retired),
                  static_cast<long long>(live), static_cast<long long>(cap));
  }
  hipMemGenericAllocationHandle_t h{};
  if ((e = hipMemCreate(&h, size, &prop, 0)) != hipSuccess)
    return fail(-static_cast<int>(e), "dol_bank_alloc: hipMemCreate(%zu): %s", size, hipGetErrorString(e));
  void* va = nullptr;
  if ((e = hipMemAddressReserve(&va, size, gran, nullptr, 0)) != hipSuccess) {
    (void)hipMemRelease(h);
    return fail(-static_cast<int>(e), "dol_bank_alloc: hipMemAddressReserve: %s", hipGetErrorString(e));
  }
  if ((e = hipMemMap(va, size, 0, h, 0)) != hipSuccess) {
    (void)hipMemAddressFree(va, size);
    (void)hipMemRelease(h);
    return fail(-static_cast<int>(e), "dol_bank_alloc: hipMemMap: %s", hipGetErrorString(e));
  }
  hipMemAccessDesc acc{};
  acc.location = prop.location;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  if ((e = hipMemSetAccess(va, size, &acc, 1)) != hipSuccess) {
    (void)hipMemUnmap(va, size);
    (void)hipMemAddressFree(va, size);
    (void)hipMemRelease(h);
    return fail(-static_cast<int>(e), "dol_bank_alloc: hipMemSetAccess: %s", hipGetErrorString(e));
  }
  {  // the handle lives until dol_bank_free has unmapped the range (create, map ... unmap, release)
    std::lock_guard<std::mutex> lk(g_bank_mu);
    g_bank_handles[va] = BankBlock{h, size};
  }
  *ptr = va;
  *mapped_bytes = static_cast<int64_t>(size);
  g_err[0] = '\0';
  return DOL_OK;
}

// Unmap, free the range, release the handle -- with the size recorded at
// allocation (mapped_bytes must match it).  The entry is erased only after all
// three succeed, so a failed step leaves the block registered and a later call
// retries from that step.
int dol_bank_free(void* ptr, int64_t mapped_bytes) {
  if (!ptr) return DOL_OK;
  std::lock_guard<std::mutex> lk(g_bank_mu);
  auto it = g_bank_handles.find(ptr);
  if (it == g_bank_handles.end()) return fail(DOL_EINVAL, "dol_bank_free: %p is not a dol_bank_alloc block", ptr);
  BankBlock& blk = it->second;
  if (mapped_bytes != static_cast<int64_t>(blk.size))
    return fail(DOL_EINVAL, "dol_bank_free: size %lld differs from the mapped %zu bytes",
                static_cast<long long>(mapped_bytes), blk.size);
  hipError_t e = hipSuccess;
  if (blk.stage == 0) {
    if ((e = hipMemUnmap(ptr, blk.size)) != hipSuccess)
      return fail(-static_cast<int>(e), "dol_bank_free: hipMemUnmap: %s", hipGetErrorString(e));
    blk.stage = 1;
  }
  if (blk.stage == 1 && !env_int("DOL_BANK_FREE_VA", 0)) {
    // The virtual range stays reserved (retired, never handed out again): on
    // this ROCm stack a new physical allocation mapped at a range a freed block
    // used is not what the GPU then reads and writes -- stale translations of
    // the old block.  tools/vmm_remap_probe.py, 12 map/free cycles in one
    // process (profiles/r05c_vmm_remap_probe.jsonl): with the range freed and
    // re-used, 7 of 11 re-mapped cycles returned wrong mix results; with the
    // range retired, or with nothing freed, all 12 were bit-exact.  A stale
    // translation to a released range is also the r04k illegal-address fault.
    // Retiring costs address space only (the physical memory is released).
    // DOL_BANK_FREE_VA=1 restores the freeing order (diagnostics only).
    // Counted in g_bank_retired (dol_bank_retired_bytes) against the cap that
    // dol_bank_alloc enforces.
    blk.stage = 2;
    g_bank_retired += static_cast<int64_t>(blk.size);
    g_bank_retired_blocks += 1;
  }
  if (blk.stage == 1) {
    if ((e = hipMemAddressFree(ptr, blk.size)) != hipSuccess)
      return fail(-static_cast<int>(e), "dol_bank_free: hipMemAddressFree: %s", hipGetErrorString(e));
    blk.stage = 2;
  }
  if ((e = hipMemRelease(blk.handle)) != hipSuccess)
    return fail(-static_cast<int>(e), "dol_bank_free: hipMemRelease: %s", hipGetErrorString(e));
  g_bank_handles.erase(it);
  g_err[0] = '\0';
  return DOL_OK;
}

int dol_stream_copy_f32(const float* src, float* dst, int64_t n, hipStream_t s) {
  DOL_DIMS_OK("dol_stream_copy_f32", n);
  DOL_CHECKED(check_rows("dol_stream_copy_f32", n < 0, n == 0, !src || !dst, false, false));
  if (aligned16(src) && aligned16(dst)) {
    const int64_t n4 = n / 4;
    if (n4 > 0) {
      const int64_t grid = cdiv(n4, int64_t(kThreads) * 4);
      if (grid > kMaxBlocks * 8) return fail(DOL_EINVAL, "dol_stream_copy_f32: too large");
      hipLaunchKernelGGL(copy_kernel, dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s,
                         reinterpret_cast<const f4*>(src), reinterpret_cast<f4*>(dst), n4);
    }
    if (n % 4)
      hipLaunchKernelGGL(copy_scalar_kernel, dim3(1), dim3(kThreads), 0, s, src + 4 * n4, dst + 4 * n4, n % 4);
  } else {
    hipLaunchKernelGGL(copy_scalar_kernel, dim3(2048), dim3(kThreads), 0, s, src, dst, n);
  }
  return check_launch("dol_stream_copy_f32");
}

}  // extern "C"
