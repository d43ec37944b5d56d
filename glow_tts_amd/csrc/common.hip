// Library identification for libglowtts_hip.so (see include/glowtts_hip.h).
#include <hip/hip_runtime.h>
#include <string.h>
#include <atomic>
#include <stdio.h>
#include "../../include/glowtts_hip.h"
#include "launch_log.h"
#include "device_common.h"

extern "C" int glowtts_abi_version(void) { return GLOWTTS_ABI_VERSION; }

extern "C" int glowtts_device_arch(char* buf, int buflen)
{
    if (!buf || buflen < 2) return GLOWTTS_E_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) { buf[0] = 0; return GLOWTTS_E_LAUNCH; }
    strncpy(buf, prop.gcnArchName, buflen - 1);
    buf[buflen - 1] = 0;
    return GLOWTTS_OK;
}

// ---- launch log (see launch_log.h) ----
namespace {
constexpr int LOG_SLOTS = 1024;        // (128 filled up in a full test-suite process once round 6 added its kernel classes: later classes went uncounted)
struct Slot { char name[96]; std::atomic<long long> n; };
Slot g_slots[LOG_SLOTS];
std::atomic<int> g_used{0};
std::atomic_flag g_lock = ATOMIC_FLAG_INIT;

Slot* find_slot(const char* cls, bool create)
{
    int used = g_used.load(std::memory_order_acquire);
    for (int i = 0; i < used; ++i) if (!strcmp(g_slots[i].name, cls)) return &g_slots[i];
    if (!create) return nullptr;
    while (g_lock.test_and_set(std::memory_order_acquire)) {}
    used = g_used.load(std::memory_order_acquire);
    Slot* s = nullptr;
    for (int i = 0; i < used; ++i) if (!strcmp(g_slots[i].name, cls)) { s = &g_slots[i]; break; }
    if (!s && used < LOG_SLOTS) {
        s = &g_slots[used];
        strncpy(s->name, cls, sizeof(s->name) - 1); s->name[sizeof(s->name) - 1] = 0; s->n.store(0);
        g_used.store(used + 1, std::memory_order_release);
    }
    g_lock.clear(std::memory_order_release);
    return s;
}
}  // namespace

std::atomic<long long>* glowtts_launch_slot(const char* cls)
{
    Slot* s = find_slot(cls, true);
    return s ? &s->n : nullptr;
}

void glowtts_note_launch(const char* cls)
{
    if (Slot* s = find_slot(cls, true)) s->n.fetch_add(1, std::memory_order_relaxed);
}

extern "C" int64_t glowtts_launch_count(const char* kernel_class)
{
    if (!kernel_class) return -1;
    // prefix match: "conv_dma<LINEAR,5" counts every NI / wave variant of that class
    long long total = 0; const size_t len = strlen(kernel_class);
    const int used = g_used.load(std::memory_order_acquire);
    for (int i = 0; i < used; ++i) if (!strncmp(g_slots[i].name, kernel_class, len)) total += g_slots[i].n.load(std::memory_order_relaxed);
    return total;
}

extern "C" void glowtts_launch_log_reset(void)
{
    const int used = g_used.load(std::memory_order_acquire);
    for (int i = 0; i < used; ++i) g_slots[i].n.store(0, std::memory_order_relaxed);
}

extern "C" int glowtts_launch_log_dump(char* buf, int buflen)
{
    if (!buf || buflen < 2) return GLOWTTS_E_ARG;
    int off = 0; buf[0] = 0;
    const int used = g_used.load(std::memory_order_acquire);
    for (int i = 0; i < used; ++i) {
        const long long n = g_slots[i].n.load(std::memory_order_relaxed);
        if (!n) continue;
        const int w = snprintf(buf + off, buflen - off, "%s %lld\n", g_slots[i].name, n);
        if (w < 0 || w >= buflen - off) break;
        off += w;
    }
    return GLOWTTS_OK;
}

// ---- sustained matrix clock (measurement aid for bench.py's roofline, see include/glowtts_hip.h) ----
namespace {
__global__ __launch_bounds__(256) void mfma_clock_probe_kernel(long long* out, int iters)
{
    // four independent accumulators per wave, one wave per SIMD: the matrix pipe issues back to back (32 clk per MFMA), operands are
    // pseudo-random bf16 (zero operands draw less power and clock higher)
    f32x16 acc[4] = {};
    bf16x8 a, b;
    uint32_t h = threadIdx.x * 0x9E3779B1u + blockIdx.x * 0x85EBCA6Bu + 12345u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12;
        a[k] = (__bf16)((float)(h & 0xFFFF) * (1.f / 32768.f) - 1.f);
        b[k] = (__bf16)((float)(h >> 16) * (1.f / 32768.f) - 1.f);
    }
    const long long c0 = clock64(), w0 = wall_clock64();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[j], 0, 0, 0);
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += acc[j][r];
    const long long c1 = clock64(), w1 = wall_clock64();
    if (threadIdx.x == 0) { out[2 * blockIdx.x] = c1 - c0 + (s == 12345.678f); out[2 * blockIdx.x + 1] = w1 - w0; }
}
}  // namespace

__global__ void stamp_kernel(long long* slot) { if (threadIdx.x == 0) *slot = wall_clock64(); }

extern "C" int glowtts_debug_stamp(long long* slot, void* stream)
{
    if (!slot) return GLOWTTS_E_ARG;
    hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), slot);
    RET_LAUNCH();
}

// One 31-bit dropout seed word per training step from a counter in device memory (see glowtts_step_seed in the header)
__global__ void step_seed_kernel(uint32_t* state, uint32_t* out)
{
    if (threadIdx.x == 0) {
        const uint32_t c = state[0] + 1u;
        state[0] = c;
        uint32_t h = state[1] + c * 0x9E3779B9u;
        h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;      // fmix (device_common.h) spelled out: the call compiles to other machine code here
        out[0] = h & 0x7FFFFFFFu;
    }
}

extern "C" int glowtts_step_seed(uint32_t* state, uint32_t* out, void* stream)
{
    if (!state || !out) return GLOWTTS_E_ARG;
    hipLaunchKernelGGL(step_seed_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), state, out);
    RET_LAUNCH();
}

extern "C" int glowtts_mfma_clock_probe(long long* out, int nwg, int iters, int* wall_khz, void* stream)
{
    if (!out || nwg <= 0 || iters <= 0) return GLOWTTS_E_ARG;
    if (wall_khz) {
        int dev = 0, khz = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return GLOWTTS_E_LAUNCH;
        *wall_khz = khz;
    }
    GLOWTTS_NOTE_STATIC("mfma_clock_probe");
    hipLaunchKernelGGL(mfma_clock_probe_kernel, dim3(nwg), dim3(256), 0, static_cast<hipStream_t>(stream), out, iters);
    RET_LAUNCH();
}
