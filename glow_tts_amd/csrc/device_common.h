// The one home of the generic device helpers of csrc/: vector types, wave reductions, bf16 pack / bits / unpack, the murmur3 finalizer and every dropout
// hash built on it (the forward and backward epilogues, and tests/dropout_masks.py, must agree on them bit for bit), the f32 MFMA wrapper, sigmoid and
// transcendental wrappers, the LDS slot swizzle and row stride, compile-time loops, buffer descriptors and the 32x32 accumulator's row map.  Every .hip / .h
// that needs one of these includes this file; what is specific to one kernel family stays in wavenet_common.h / ge2e_common.h / pwg_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

typedef u32x4 Chunk16;                                             // one 16-byte LDS slot (native vector: stays in VGPRs)

// sum / maximum over the 64 lanes in a fixed tree (xor 32, 16, ... 1): every lane ends with the same value
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// bf16 (round to nearest even): two values packed into one word, the bits of one value, and a bf16's bits back to f32
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return *reinterpret_cast<uint32_t*>(&v);
}
__device__ __forceinline__ uint16_t bf16_bits(float v) { const __bf16 b = (__bf16)v; return *reinterpret_cast<const uint16_t*>(&b); }
__device__ __forceinline__ float bf16_to_f32(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

__device__ __forceinline__ int swz(int row, int q) { return row * 64 + ((q ^ ((row >> 2) & 3)) << 4); }

// the 4-pass bf16 instruction: A = 16 rows x 32 k (lane = (row & 15, k slot lane >> 4)), B = 16 columns x 32 k, C element i = row 4 (lane >> 4) + i,
// column lane & 15.  A SIMD keeps issuing vector-memory instructions between these; between back-to-back 32x32x16 MFMAs it does not (tools/wn_lab.hip)
template <bool ON = true>
__device__ __forceinline__ f32x4 mfma16_bf16(const Chunk16& a, const Chunk16& b, const f32x4& c) {
    if constexpr (!ON) { f32x4 r = c; r[0] += __uint_as_float(a[0] ^ b[0]); return r; }
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(&a), *reinterpret_cast<const bf16x8*>(&b), c, 0, 0, 0);
}
// LDS slot swizzle of [rows][64 B] tiles read as 16x16x32 fragments: bank-conflict free for ds_read_b128 at any row shift (period 8 rows)
__device__ __forceinline__ int swz16(int row, int q) { return row * 64 + ((q ^ (((row >> 2) & 1) << 1)) << 4); }
// Fragment reads the COMPILER DOES NOT SEE (inline asm), paired with a hand-placed counted wait: hipcc's own s_waitcnt insertion puts lgkmcnt(0) in front
// of the MFMAs of slab j where lgkmcnt(6) is meant (the six reads of slab j + 1, issued right before, may stay in flight) - the software pipeline then
// waits out an LDS round trip every other slab.  `addr`: LDS byte address; OFF: immediate offset (< 65536).  lgkm_wait<N>(a, b) waits until at most N
// LGKM operations are outstanding and is tied to the fragment registers, so no use of them can be scheduled in front of it.
template <int OFF> __device__ __forceinline__ Chunk16 lds16_asm(uint32_t addr) {
    Chunk16 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
    return v;
}
template <int N> __device__ __forceinline__ void lgkm_wait(Chunk16 (&a)[2], Chunk16 (&b)[4]) {
    asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]) : "n"(N));
}
template <int N> __device__ __forceinline__ void lgkm_wait(Chunk16 (&a)[2], Chunk16 (&b)[2]) {
    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]) : "n"(N));
}
template <int N> __device__ __forceinline__ void lgkm_wait(Chunk16 (&a)[2], Chunk16 (&b)[6]) {
    asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(a[0]), "+v"(a[1]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]) : "n"(N));
}
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char*)p; }

// EXACT = f32 mode: libm-grade transcendental functions; bf16 mode: hardware exp (v_exp_f32)
template <bool EXACT> __device__ __forceinline__ float exp_(float x) { return EXACT ? expf(x) : __expf(x); }
template <bool EXACT> __device__ __forceinline__ float rcp_(float x) { return EXACT ? 1.f / x : __builtin_amdgcn_rcpf(x); }
template <bool EXACT> __device__ __forceinline__ float sigmoid_(float x) { return rcp_<EXACT>(1.f + exp_<EXACT>(-x)); }
template <bool EXACT> __device__ __forceinline__ float tanh_(float x) {
    if (EXACT) return tanhf(x);
    const float e = __expf(2.f * x);          // tanh(x) = 1 - 2 / (exp(2x) + 1)
    return 1.f - 2.f * __builtin_amdgcn_rcpf(e + 1.f);
}

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }
// one v_mfma_f32_16x16x4_f32: lane (r = lane & 15, q = lane >> 4) holds A[r][q] and B[q][r]; C element i = row 4 q + i, column r
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
// row stride (floats) of an LDS tile of K floats per row read as mfma4 operands: (stride / 4) odd, so 16 rows x 4 k hit distinct banks
__host__ __device__ __forceinline__ int lds_stride_of(int K) { return ((K >> 2) & 1) ? K : K + 4; }
// row of element `reg` of a 32x32 MFMA accumulator held by a lane with lhi = lane >> 5
__host__ __device__ constexpr int acc_row(int reg, int lhi) { return (reg & 3) + 8 * (reg >> 2) + 4 * lhi; }

// f(IC<0>{}), f(IC<1>{}), ... f(IC<N - 1>{}): straight-line code over compile-time step numbers
template <int V> struct IC { static constexpr int value = V; };
template <int N> struct StaticFor {
    template <class F> __device__ __forceinline__ static void run(F&& f) { StaticFor<N - 1>::run(f); f(IC<N - 1>{}); }
};
template <> struct StaticFor<0> { template <class F> __device__ __forceinline__ static void run(F&&) {} };

// raw buffer descriptor of `bytes` bytes at `ptr`: loads beyond it return zero, stores beyond it are dropped
typedef __amdgpu_buffer_rsrc_t Rsrc;
__device__ __forceinline__ Rsrc mk_rsrc(const void* ptr, long bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, (int)bytes, 0x00020000); }

// The murmur3 finalizer, split at its second multiply: every hash of the library (dropout, the step seed, gauss_hash.h) is built from these two halves
__host__ __device__ __forceinline__ uint32_t fmix_head(uint32_t h) { h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; return h; }
__host__ __device__ __forceinline__ uint32_t fmix_tail(uint32_t h) { h *= 0xC2B2AE35u; return h ^ (h >> 16); }
__host__ __device__ __forceinline__ uint32_t fmix(uint32_t h) { return fmix_tail(fmix_head(h)); }

// Dropout of the WaveNet gate pre-activations (Modules.py:862).  The GATE (forward) and DGATE (backward) epilogues must draw the
// same mask, and integer multiplies are quarter rate, so: one key per row (2 multiplies), one 32-bit draw per (row, channel
// pair) (1 multiply) whose low / high 16 bits decide the tanh / the sigmoid channel.  keep <=> half >= thr, thr = round(p * 2^16);
// kept values are scaled by 2^16 / (2^16 - thr), the exact inverse keep rate of that threshold.
__device__ __forceinline__ uint32_t drop_threshold(float p) { return p > 0.f ? (uint32_t)(p * 65536.f + 0.5f) : 0u; }
__device__ __forceinline__ float drop_inv_keep(uint32_t thr) { return 65536.f / (65536.f - (float)thr); }
__device__ __forceinline__ uint32_t drop_rowkey(uint32_t seed, uint32_t r) { return fmix_head(r * 0x9E3779B1u + seed); }
__device__ __forceinline__ uint32_t drop_colkey(uint32_t j) { return (j + 1u) * 0x27D4EB2Fu; }
__device__ __forceinline__ uint32_t drop_draw(uint32_t rowkey, uint32_t colkey) { return fmix_tail(rowkey ^ colkey); }
__device__ __forceinline__ float drop_keep_lo(uint32_t d, uint32_t thr, float ik) { return (d & 0xFFFFu) >= thr ? ik : 0.f; }
__device__ __forceinline__ float drop_keep_hi(uint32_t d, uint32_t thr, float ik) { return (d >> 16) >= thr ? ik : 0.f; }

// dropout keep decision of the text encoder's sites (the LINEAR epilogue, proj_ln, LayerNorm, attention): counter hash of (seed, element id) -> 24-bit uniform
__device__ __forceinline__ float drop_scale(uint32_t seed, uint32_t id, float p, float inv_keep) {
    const uint32_t h = fmix(id * 0x9E3779B1u + seed);
    return ((h >> 8) * (1.0f / 16777216.0f) >= p) ? inv_keep : 0.f;
}


}  // namespace

// Conditioning-gradient accumulators (round 5): fixed point, units of 2^-40, 64-bit integer atomics.  Integer addition commutes, so the per-utterance sums that the
// workgroups of a launch (and the launches of the twelve flows' layers) add into one buffer no longer depend on the order they arrive in: the gradients of the
// Speaker_l / Prosody_l / Pitch_l convs are bit-reproducible from run to run (fp32 atomic adds were not).  Range +- 2.1e6 (beyond: poisoned, below), resolution 9.1e-13 per addend.
constexpr float GLOWTTS_FX_SCALE = 1099511627776.f;          // 2^40
// A non-finite addend, or one beyond +- 2^21 (2^61 units - a quarter of the range), POISONS the accumulator instead of vanishing in the float -> integer conversion
// (NaN -> 0, Inf -> saturation): it is set to the largest value, later addends only move it within |acc| >= 2^61, and glowtts_fx_to_float (cond_ops.hip)
// reads such an accumulator as NaN - the Speaker_l / Prosody_l / Pitch_l gradients propagate a diverging step like fp32 sums did.
constexpr long long GLOWTTS_FX_POISON = 0x2000000000000000LL;        // 2^61
__device__ __forceinline__ void fx_atomic_add(long long* dst, float v) {
    const float s = v * GLOWTTS_FX_SCALE;
    if (!(fabsf(s) < 2.3e18f)) { atomicExch(reinterpret_cast<unsigned long long*>(dst), 0x7FFFFFFFFFFFFFFFull); return; }
    atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)__float2ll_rn(s));
}

