// launch_util.h -- per-device launch state shared by the kernel launchers.
//
// The C ABI is re-entrant (include/nerf_amd.h): any host thread may launch on any device.  What a
// launcher remembers between calls is therefore kept per device and updated atomically:
//   * whether a kernel's dynamic-LDS limit has been raised on a device (hipFuncSetAttribute is a
//     per-device property of the loaded code object),
//   * a device's CU count,
//   * a device's pool of {ticket, done} pairs for the kernels that deal their tiles dynamically.
// On top of that state: the table of the fused field family (for_family) and the one launch path of its kernels
// (launch_field).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>

#include "kernels.h"

namespace na {

extern std::atomic<int> g_variant;    // nerf_amd_set_tuning key 0 (A/B selection; relaxed loads in the launchers); capi.hip

constexpr int MAX_TRACKED_DEVICES = 64;

inline int current_device() {
    int d = 0;
    return hipGetDevice(&d) == hipSuccess ? d : -1;
}

// CU count of the current device (cached per device; 256 if the query fails).
inline int device_cu_count() {
    static std::atomic<int> cache[MAX_TRACKED_DEVICES];      // zero-initialised
    const int dev = current_device();
    const bool tracked = dev >= 0 && dev < MAX_TRACKED_DEVICES;
    if (tracked) {
        const int c = cache[dev].load(std::memory_order_relaxed);
        if (c > 0) return c;
    }
    int n = 0;
    if (dev < 0 || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    if (tracked) cache[dev].store(n, std::memory_order_relaxed);
    return n;
}

// One object per kernel instantiation (a function-local static of the launcher template): the set of
// devices on which the kernel's dynamic-LDS limit has been raised.  Two threads racing on the same
// device both call hipFuncSetAttribute with the same value, which is harmless.
struct DynamicLdsOptIn {
    std::atomic<uint64_t> done{0};
    hipError_t ensure(const void *kernel, size_t bytes) {
        const int dev = current_device();
        const bool tracked = dev >= 0 && dev < MAX_TRACKED_DEVICES;
        const uint64_t bit = tracked ? (uint64_t)1 << dev : 0;
        if (tracked && (done.load(std::memory_order_acquire) & bit)) return hipSuccess;
        const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e == hipSuccess && tracked) done.fetch_or(bit, std::memory_order_release);
        return e;
    }
};

// ---- the fused field family (D=8, W=256, skips=[4]): the models the fused kernels are instantiated for
template <int LX, int LD, bool VD>
struct Family {
    static constexpr int lx = LX, ld = LD;      // multires, multires_views (0 without view branch)
    static constexpr bool vd = VD;              // view branch
};

// f(Family<...>{}) for the family of (multires, multires_views, use_viewdirs); NERF_AMD_EUNSUPPORTED outside the table.
template <class F>
int for_family(int multires, int multires_views, int use_viewdirs, F &&f) {
    if (use_viewdirs) {
        if (multires == 10 && multires_views == 4) return f(Family<10, 4, true>{});
        if (multires == 15 && multires_views == 6) return f(Family<15, 6, true>{});
    } else {
        if (multires == 10) return f(Family<10, 0, false>{});
        if (multires == 15) return f(Family<15, 0, false>{});
    }
    return NERF_AMD_EUNSUPPORTED;
}
inline bool family_known(int multires, int multires_views, int use_viewdirs) {
    return for_family(multires, multires_views, use_viewdirs, [](auto) { return NERF_AMD_OK; }) == NERF_AMD_OK;
}
// Every fused kernel but the first-generation one (mlp_bf16.hip) keeps the head of an output_linear model in one 16-row tile.
constexpr bool head_fits(bool view_branch, int out_ch) { return view_branch || out_ch <= 16; }
// The fused programs exist (D=8, W=256, skips=[4]) and the kernels generate the positional encoding themselves.
inline bool fused_program(const Program &p) { return p.bf16_ok && p.arch.i_embed == 0; }

// ---- {ticket, done} pairs of the dynamic deal (defined in capi.hip)
// A pair for one launch of a kernel that deals its tiles dynamically (zero between launches: the last workgroup to leave
// resets it).  Round robin over 1024 pairs per device, allocated by tile_counters_init.
unsigned *tile_counter_slot(int device);
// ... for a launch on stream s, or NULL (= the static deal) when the deal is off or s is being captured into a graph: a
// captured launch would bake its pair into every replay, and a replay may run beside an eager launch that drew the same pair
unsigned *tile_counter_for(bool deal, hipStream_t s);
int tile_counters_init(int device);

// ---- one launch path for the field kernels
// Workgroups of a launch over P points, wg_points per tile: one per tile (n_wg == 0), or at most n_wg that walk the tiles --
// blockIdx, blockIdx + gridDim, ... up to two tiles each, by ticket above that (unless tickets are switched off).
struct FieldGrid { int64_t groups; bool deal; };
constexpr FieldGrid field_grid(int64_t P, int wg_points, int64_t n_wg, bool tickets) {
    FieldGrid g{(P + wg_points - 1) / wg_points, false};
    if (n_wg > 0) {
        g.deal = g.groups > 2 * n_wg && tickets;
        if (g.groups > n_wg) g.groups = n_wg;
    }
    return g;
}

struct FieldKernel {
    const void *kernel;            // __global__ void (MlpArgs)
    DynamicLdsOptIn *opt_in;       // the instantiation's own (a function-local static of its launcher)
    size_t lds;                    // dynamic LDS bytes
    int threads, wg_points;        // workgroup size, points per tile
    int wg_per_cu;                 // 0: one workgroup per tile; n: n workgroups per CU walk the tiles (field_grid)
};
inline int launch_field(const FieldKernel &k, MlpArgs a, hipStream_t s) {
    if (k.opt_in->ensure(k.kernel, k.lds) != hipSuccess) return NERF_AMD_EHIP;
    if (a.P <= 0) return NERF_AMD_OK;
    if (a.P >= (int64_t)1 << 31) return NERF_AMD_EINVAL;
    // A/B 42: the walking kernels take their tiles blockIdx + k gridDim at every size
    const FieldGrid g = field_grid(a.P, k.wg_points, k.wg_per_cu ? (int64_t)k.wg_per_cu * device_cu_count() : 0, g_variant != 42);
    a.tile_ctr = tile_counter_for(g.deal, s);
    void *args[] = {&a};
    (void)hipLaunchKernel(k.kernel, dim3((unsigned)g.groups), dim3(k.threads), args, k.lds, s);
    return hipGetLastError() == hipSuccess ? NERF_AMD_OK : NERF_AMD_EHIP;
}

}  // namespace na
