// Internal helpers shared by the libvfx_hip translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "../../include/vfx_hip.h"

extern __attribute__((visibility("hidden"))) std::atomic<uint64_t> g_vfx_launches;

#define VFX_LAUNCHED() (g_vfx_launches.fetch_add(1, std::memory_order_relaxed))

static inline int vfx_last_error() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? VFX_OK : (int)e;
}

// Zero ``bytes`` (a multiple of 4) of device memory on a stream with a KERNEL (vfx_misc.hip), not hipMemsetAsync: see there.
// (internal: hidden visibility, not part of the C ABI)
__attribute__((visibility("hidden"))) int vfx_zero_u32(void* p, size_t bytes, hipStream_t s);

// Development switches (VFX_WINO4_D1, VFX_KC16, ...): environment variables that change WHICH kernel a launch runs.  They are read
// only by -DVFX_DEV builds (`make dev` -> libvfx_hip_dev.so, selected with VFX_LIB=...); the release library reads no
// environment variable at all, and the switch names do not appear in it (tests/test_api_cpu.py greps the .so).
#ifdef VFX_DEV
#include <stdlib.h>
#define VFX_DEV_ENV(name) getenv(name)
#else
#define VFX_DEV_ENV(name) (static_cast<const char*>(nullptr))
#endif

static inline bool vfx_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

#ifdef VFX_DEV
#include <cxxabi.h>
#include <stdio.h>
#include <string.h>
#include <typeinfo>
// Development dump of one launch (VFX_DEBUG_ARGS=1): "<kernel><template arguments> grid x y z lds n args:" and every kernel
// argument as 32-bit words.  The kernel is named after the instance this launcher was instantiated for: conv_taps_kernel<128, 128,
// 2, 2, 8, true, 4, false> prints as conv_taps<128,128,2,2,8,1,4,0>.
template <typename T>
static void vfx_dump_words(const T& v) {
    unsigned w[(sizeof(T) + 3) / 4] = {0};
    memcpy(w, &v, sizeof(T));
    for (size_t i = 0; i < sizeof(T) / 4; ++i) fprintf(stderr, " %08x", w[i]);
}
template <auto Kern>
struct VfxKernelTag {};   // its demangled name spells the instance: VfxKernelTag<&(void conv_taps_kernel<128, .., false>(ConvArgs))>
template <auto Kern, typename... Args>
static void vfx_dump_launch(dim3 grid, size_t lds, const Args&... args) {
    static const char* const tag = abi::__cxa_demangle(typeid(VfxKernelTag<Kern>).name(), nullptr, nullptr, nullptr);
    const char* p = tag ? strstr(tag, "&(") : nullptr;
    p = p ? p + 2 : "?";
    if (strncmp(p, "void ", 5) == 0) p += 5;
    for (; *p && *p != '(' && *p != '<'; ++p)
        if (strncmp(p, "_kernel", 7) == 0) p += 6; else fputc(*p, stderr);
    for (int depth = 0; *p && (depth > 0 || *p == '<'); ++p) {   // the template arguments: no blanks, bools as 1 / 0
        depth += *p == '<' ? 1 : (*p == '>' ? -1 : 0);
        if (strncmp(p, "true", 4) == 0) { fputc('1', stderr); p += 3; }
        else if (strncmp(p, "false", 5) == 0) { fputc('0', stderr); p += 4; }
        else if (*p != ' ') fputc(*p, stderr);
    }
    fprintf(stderr, " grid %u %u %u lds %zu args:", grid.x, grid.y, grid.z, lds);
    (vfx_dump_words(args), ...);
    fprintf(stderr, "\n");
}
#endif

// The one launch sequence of every kernel that takes dynamic LDS: raise the kernel's dynamic-LDS limit to the 160 KB of a gfx950 CU
// on first use per device (bit d of ``attr_set``: done on device d -- one process may drive several devices, from several host
// threads), launch, count the launch, return the launch's error.  One instantiation, and so one bitmask, per kernel instance.
template <auto Kern, typename... Args>
static int vfx_launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args&... args) {
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_relaxed) & bit)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return (int)e;
        attr_set.fetch_or(bit, std::memory_order_relaxed);
    }
#ifdef VFX_DEV
    static const bool dump = VFX_DEV_ENV("VFX_DEBUG_ARGS") && atoi(VFX_DEV_ENV("VFX_DEBUG_ARGS")) != 0;
    if (dump) vfx_dump_launch<Kern>(grid, lds, args...);
#endif
    hipLaunchKernelGGL(Kern, grid, block, lds, s, args...);
    VFX_LAUNCHED();
    return vfx_last_error();
}

__device__ __forceinline__ float vfx_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

__device__ __forceinline__ float vfx_post(float v, int act, float slope) {
    switch (act) {
        case VFX_POST_LRELU: return vfx_lrelu(v, slope);
        case VFX_POST_ELU: return v > 0.f ? v : expm1f(v);
        case VFX_POST_TANH: return tanhf(v);
        case VFX_POST_SIGMOID: return 1.f / (1.f + expf(-v));
        case VFX_POST_LRELU_SNAKE: { float u = vfx_lrelu(v, slope); return u + sinf(u); }
        default: return v;
    }
}
