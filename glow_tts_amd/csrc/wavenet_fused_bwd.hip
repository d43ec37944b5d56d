// Backward of the fused coupling network (wavenet_fused.hip) for gfx950: the DATA gradients of one flow's Start conv, WaveNet and End conv
// (autograd of Modules.py:785-806, 858-887) in ONE launch.  The weight gradients stay with the grouped wgrad launches at the end of the
// decoder backward; this kernel leaves them their operands (d skip, the gate gradients dins_l, d x_l) in global memory.
//
//   d skip = (d(m, logs) W_end^T) * mask                                              [End^T:   K = 192, 3 slabs]
//   for l = L-1 .. 0:
//     d acts = [d x_{l+1} | d skip] W_rs_l^T   (last layer: d skip only)              [RS^T:    K = 384 / 192, 6 / 3 slabs]
//     (da, ds) = d acts * (s (1 - t^2), t s (1 - s)) -> dropout mask -> dins_l        (gates (t, s) kept by the forward)
//     d x_l = (conv5^T(dins_l) + d x_{l+1}) * mask                                    [In^T:    K = 5 x 384, 30 slabs]
//   d x_a += d x_0 W_start^T                                                          [Start^T: K = 192, 2 slabs]
//
// Same machine as the forward: 12 waves, a 64-row window per workgroup whose valid region shrinks by 2 rows per layer on each side (here
// from the last layer down; 52 owned rows for L = 4), operands of the k = 5 transposed conv in LDS with their halo, all transposed weights
// of the flow as one image of 24-KiB slabs streamed through an LDS ring by LDS-DMA.  What differs:
//   * every GEMM here has 192 output columns = 6 fragments x 2 row fragments = one 32 x 32 fragment per wave.  For the large one (In^T)
//     that tiling would read 2 KiB of LDS per MFMA; instead waves work in PAIRS over the two K chunks of a slab - wave (rf, cp, kh)
//     multiplies rows rf, columns [64 cp, 64 cp + 64) over chunk kh (1.5 KiB per MFMA, as in the forward) - and the partners swap halves
//     of their partial sums through LDS after the last slab; each wave ends up with exactly its fragment (rf, 2 cp + kh).
//   * LDS budget: d x_{l+1} (24 KiB), d skip (26 KiB) and the gate gradients with their halo (384 channels x 68 rows = 52 KiB) do not fit
//     beside a ring.  In^T therefore runs in two K passes over ONE 26-KiB tile: first the tanh-side gradients da (K chunks 0..5 of the
//     un-paired transposed image), then the tile is rewritten with the sigmoid-side gradients ds (chunks 6..11) from registers (the pair is
//     kept packed as bf16x2: 16 VGPRs).  The ring has three slots (two slabs in flight).
// Arithmetic and roundings are those of the per-conv backward (bf16 d skip, dins, d x_l; fp32 d x_0): results differ by accumulation order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/glowtts_hip.h"
#include "tunable.h"
#include "launch_log.h"
#include "wavenet_common.h"

int glowtts_wavenet_safe_waits_flag();        // wavenet_fused.hip

namespace {

constexpr int BW_NS = 3;                                        // ring slots
// LDS map (bytes)
constexpr int BOFF_DX = 0;                                      // d x_{l+1}: [6][64][64] (window rows)
constexpr int BSZ_DX = WN_KCH * WN_WIN * 64;
constexpr int BOFF_DS = BOFF_DX + BSZ_DX;                       // d skip: [6][68][64] (tile rows = window rows - 2 .. + 66)
constexpr int BSZ_T = WN_KCH * WN_XR * 64;
constexpr int BOFF_DT = BOFF_DS + BSZ_T;                        // da or ds of the layer: [6][68][64]; before that: d(m, logs) rows
constexpr int BOFF_RING = BOFF_DT + BSZ_T;
constexpr int BOFF_MK = BOFF_RING + BW_NS * WN_SLAB;
constexpr int BOFF_UT = BOFF_MK + WN_XR * 4;                    // utterance of the 68 tile rows (conditioned models)
constexpr int BOFF_P3 = BOFF_UT + WN_XR * 4;                    // sigmoid-side gate gradients of tile rows 64..67 (last layer), parked until the second pass: [6][4][64 B]
constexpr int BW_LDS = BOFF_P3 + WN_KCH * 4 * 64;
static_assert(BW_LDS <= 160 * 1024, "LDS budget");
static_assert(BSZ_T >= WN_NW * 8 * 256, "the partial-sum exchange (8 registers per wave and round) reuses the gate-gradient tile");

struct wn_bwd_args {
    int rows, rows_per_utt, L, C2;
    const unsigned char* wimg;                    // transposed weight image of the flow
    const void* douts_bf; int64_t ldo;            // [rows][ldo] bf16 PAIR-packed d(m, logs), pad columns zero
    const float* rowmask;
    const void* gates[WN_MAXL];                   // kept (t, s) pairs, bf16 [rows][2 H]
    float drop_p; uint32_t seed; const uint32_t* seed_ptr;
    void* dskip;                                  // out: bf16 [rows][H]
    void* dins[WN_MAXL]; int64_t ldin;            // out: bf16 [rows][ldin] PAIR-packed (da | ds per 32 channels)
    void* dh[WN_MAXL];                            // out: d x_l, l >= 1 bf16 [rows][H]; l = 0 fp32 [rows][H] (bf16 like the others when dh0_bf16)
    int dh0_bf16;
    float* dx; int64_t lddx;                      // in / out: [rows][lddx] fp32, channels [0, C2) += d x_a
    float* dcond; int64_t ldcond;                 // COND: d conditioning [utterances][ldcond] as 64-bit FIXED-POINT accumulators (2^-40 units; the pointer's type is nominal), layer l at + l * 2 H; ACCUMULATED (integer atomic adds: order-independent)
    long long* tl;                                // tools builds (ABL & 64): per-workgroup phase stamps [grid][64]
    int stagger;                                  // experiment (tools builds): start delay of workgroup b = ((b >> 3) & 7) * stagger * 512 clocks
};

// COND: the per-utterance conditioning joins the gate pre-activation AFTER the dropout (Modules.py:861-866): its gradient is the sum over an
// utterance's rows of (da, ds) BEFORE the keep mask, which only exists here in registers.  Every workgroup adds the sums of its OWNED rows to
// dcond with 64-bit fixed-point atomic adds, one run per utterance (as the per-conv DGATE epilogue does; integer adds: bit-reproducible).
// ABL (tools builds only, tools/bench_wn.py): timing ablations - 1: no weight DMAs after the prologue, 2: no MFMAs, 4: no global stores (copy-outs, d x_0, d x_a),
// 8: no gate loads, 16: no partial-sum exchange, 64: per-workgroup phase stamps (s_memtime of thread 0; results stay right).  1..16: wrong results by design.
//
// Round 5: rebuilt on the forward kernel's footing (wavenet_fused.hip, round 4).  Every product runs on v_mfma_f32_16x16x32_bf16 - between
// back-to-back 8-pass 32x32x16 MFMAs a SIMD issues no vector-memory instruction, so weight DMAs and matrix work added up instead of overlapping -
// on `swz16` tiles (conflict-free ds_read_b128 at every tap shift) with the source-side DMA swizzle that goes with them; the 30 slab steps of
// In_l^T are straight-line code whose fragment reads are inline asm with hand-counted lgkmcnt waits (slab j's reads fly under slab j - 1's MFMAs;
// the compiler's own waits fall back to lgkmcnt(0) at every block boundary), `last` is a compile-time parameter of the layer body for the same reason;
// the wave pairs swap their partial sums in ONE round (two barriers instead of four: 8 registers through the gate-gradient tile, 8 through the ring
// slot the layer's last slab has just left).  Accumulator element i of fragment (rt, ct) of a wave: row 16 rt + 4 (lane >> 4) + i, column
// 16 ct + (lane & 15).
template <bool DROP, bool COND, int ABL = 0>
__global__ __launch_bounds__(WN_NT) void wn_bwd_kernel(const wn_bwd_args p)
{
    extern __shared__ __attribute__((aligned(1024))) unsigned char wb_smem[];
    unsigned char* const DX = wb_smem + BOFF_DX;
    unsigned char* const DS = wb_smem + BOFF_DS;
    unsigned char* const DT = wb_smem + BOFF_DT;
    float* const MK = reinterpret_cast<float*>(wb_smem + BOFF_MK);
    int* const UT = reinterpret_cast<int*>(wb_smem + BOFF_UT);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int rf = wave >= 6 ? 1 : 0, cf = wave - rf * 6;      // one-fragment GEMMs: this wave's 32 rows x 32 columns (row half rf, 32-channel block cf)
    const int cp = cf >> 1, kh = cf & 1;                       // In^T: 64-column block of the wave pair / K chunk of this wave
    const int L = p.L;
    const int halo = WN_PAD * (L - 1);
    const int nvalid = WN_WIN - 2 * halo;
    const int v0 = blockIdx.x * nvalid;                        // first owned row
    const int t0 = v0 - halo;                                  // global row of window row 0
    const int xr0 = t0 - WN_PAD;                               // global row of tile row 0
    const int lim = (p.rows - v0) < nvalid ? (p.rows - v0) : nvalid;
    const int jch0 = cf * 32 + l15;                            // this lane's channels in 192-wide tensors: jch0 and jch0 + 16

    // ---- weight stream (see wavenet_fused.hip): slab s -> ring slot s % 3; this wave's two 1-KiB units are rows [32 wave, 32 wave + 32) of the slab;
    // lane i of a unit lands in LDS row i >> 2, slot i & 3, and fetches the global slot (i & 3) ^ swizzle(row) ----
    const int lrow = lane >> 2, qa = (lane & 3) ^ (((lane >> 4) & 1) << 1);
    const unsigned char* const wsrc = p.wimg + (uint32_t)((wave * 32 + lrow) * 64 + qa * 16);
    auto issue = [&](int s) __attribute__((always_inline)) {
        const unsigned char* src = wsrc + (size_t)s * WN_SLAB;
        unsigned char* dst = wb_smem + BOFF_RING + (s % BW_NS) * WN_SLAB + wave * 2048;
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)src, (void __attribute__((address_space(3)))*)dst, 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(src + 1024), (void __attribute__((address_space(3)))*)(dst + 1024), 16, 0, 0);
    };
    int snext = 0;
    int tli = 0;
    auto TLS = [&]() __attribute__((always_inline)) { if constexpr ((ABL & 64) != 0) { if (tid == 0) p.tl[blockIdx.x * 64 + tli] = (long long)__builtin_readcyclecounter(); ++tli; } };
    TLS();
    // A slab step: begin_step(IC<X>) = this wave's DMAs of slab `snext` have landed, barrier (everyone's have, everyone is done with slab snext - 1) ->
    // its slot.  X = vector-memory operations this wave has issued BEHIND the DMAs of slab snext besides the two DMAs of slab snext + 1 (memory
    // operations retire in order on vmcnt, loads and stores alike on gfx9): the prefetched gate loads and the copy-outs' stores.  vmcnt(2 + X) waits
    // for exactly slab snext; a smaller count would also wait for the wave's own stores to be acknowledged / its gate loads to return.  X must never
    // exceed the real count: every counted operation is an unconditional buffer instruction.  The conditioned variants (their atomics make the
    // count data-dependent) run the conservative vmcnt(2) everywhere.  The last two slabs (Start^T) drain the ring with conservative counts.
    constexpr bool EXACT = !COND && !(ABL & 128);              // (ABL & 128: the test hook glowtts_wavenet_debug_safe_waits - conservative counts, same bits)
    auto begin_step = [&](auto X_) __attribute__((always_inline)) -> const unsigned char* {
        constexpr int X = EXACT ? decltype(X_)::value : 0;
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(2 + X) : "memory");
        return wb_smem + BOFF_RING + (snext % BW_NS) * WN_SLAB;
    };
    constexpr int XC = 2;                                      // stores of a copy_out
    auto end_step = [&]() __attribute__((always_inline)) {
        if (!(ABL & 1)) issue(snext + BW_NS - 1);
        ++snext;
    };
    auto plain_barrier = [&]() __attribute__((always_inline)) { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

    // ---- prologue: d(m, logs) rows of the tile -> DT (A operand of End^T), row masks ----
    issue(0); issue(1);
#ifdef GLOWTTS_TOOLS
    for (int k = 0; k < (int)((blockIdx.x >> 3) & 7) * p.stagger; ++k) __builtin_amdgcn_s_sleep(8);
#endif
    {
        const int per_row = (WN_H * 2) / 16;                   // 24 16-byte pieces per row (ldo = 192)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int idx = tid + k * WN_NT;
            if (idx < WN_XR * per_row) {
                const int i = idx / per_row, pc = idx - i * per_row;
                int g = xr0 + i;
                g = g < 0 ? 0 : (g >= p.rows ? p.rows - 1 : g);
                const Chunk16 v = *reinterpret_cast<const Chunk16*>(static_cast<const unsigned char*>(p.douts_bf) + ((int64_t)g * p.ldo) * 2 + pc * 16);
                *reinterpret_cast<Chunk16*>(DT + (pc >> 2) * (WN_XR * 64) + swz16(i, pc & 3)) = v;
            }
        }
        if (tid < WN_XR) {
            int g = xr0 + tid;
            g = g < 0 ? 0 : (g >= p.rows ? p.rows - 1 : g);
            MK[tid] = p.rowmask[g];
            if (COND) UT[tid] = g / p.rows_per_utt;
        }
    }
    const int bl = swz16(l15, lq);                             // per-lane fragment offset: row l15 of a 16-row block (+1024 B per block), slot lq
    const int offA = rf * 2048;                                // this wave's 32-row half of a tile chunk
    const int rbw = rf * 32 + 4 * lq;                          // first tile / window row of this lane's accumulator rows (rt = 0, i = 0)
    // byte offset inside a 64-byte tile row of channel 16 h + l15 of a 32-channel chunk, for a row whose (row >> 2) parity is (lq + cy) & 1
    auto tile_off_of = [](int l15x, int lqx, int h, int cy) __attribute__((always_inline)) -> int {
        return ((((2 * h + (l15x >> 3)) ^ (((lqx + cy) & 1) << 1)) & 3) << 4) + (l15x & 7) * 2;
    };
    // Every phase derives its per-lane addresses from an OPAQUE copy of the lane id: all of them are invariant over the layers, and left alone the
    // compiler hoists them out of the layer loop and keeps dozens of registers live across the GEMM loops (the first build of this kernel spilled).
    auto fresh_lane = [&]() __attribute__((always_inline)) -> int { int a = lane; asm volatile("" : "+v"(a)); return a; };

    // copy of the owned rows of an LDS tile [6 chunks][trows][64 B] to global rows: piece (chunk kc, slot q) of row r goes to
    // dst + r * row_bytes + off + kc * chunk_bytes + 16 q
    auto copy_out = [&](const unsigned char* tile, int trows, int row_off, void* dst, int row_bytes, int chunk_bytes, int off) __attribute__((always_inline)) {
        if constexpr ((ABL & 4) != 0) return;
        const Rsrc rd = mk_rsrc(dst, (long)p.rows * row_bytes);
        int tid_ = tid;
        asm volatile("" : "+v"(tid_));
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int idx = tid_ + k * WN_NT;
            const int r = idx / 24, pc = idx - r * 24;
            const bool ok = r < lim;
            const Chunk16 v = lds16(tile + (pc >> 2) * (trows * 64) + swz16(row_off + (ok ? r : 0), pc & 3));
            __builtin_amdgcn_raw_buffer_store_b128(v, rd, ok ? (uint32_t)((v0 + r) * row_bytes + off + (pc >> 2) * chunk_bytes + (pc & 3) * 16) : OOB, 0, 0);
        }
    };

    f32x4 acc[2][4];                                           // [16-row fragment rt][16-column fragment ct]
    f32x4 a3[2];                                               // third row fragment (tile rows 64..79, of which 64..67 exist) of the waves rf = 0: [ct]
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        a3[0] = a3[1] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // one-fragment GEMM step over a slab of two K chunks x 192 columns: A chunk tiles a0 / a1 ([rows][64 B]), this wave's rows start at tile row
    // 32 rf + shift (shift 0: one lane offset serves both fragments); `third`: rows 64..79 of the same tiles into a3 (waves rf = 0)
    auto mma192 = [&](const unsigned char* slot, const unsigned char* a0, const unsigned char* a1, bool third, int shift) __attribute__((always_inline)) {
        Chunk16 fa[2][2], fb[2][2], f3[2];
        int ar0 = offA + bl, ar1 = offA + 1024 + bl;
        if (shift) {
            const int ln = fresh_lane();
            ar0 = swz16(rf * 32 + (ln & 15) + shift, ln >> 4);
            ar1 = swz16(rf * 32 + 16 + (ln & 15) + shift, ln >> 4);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const unsigned char* At = c ? a1 : a0;
            fa[c][0] = lds16(At + ar0);
            fa[c][1] = lds16(At + ar1);
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) fb[c][ct] = lds16(slot + c * 12288 + cf * 2048 + ct * 1024 + bl);
            if (third) f3[c] = lds16(At + 4096 + bl);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = mfma16_bf16<!(ABL & 2)>(fa[c][rt], fb[c][ct], acc[rt][ct]);
            if (third) {
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) a3[ct] = mfma16_bf16<!(ABL & 2)>(f3[c], fb[c][ct], a3[ct]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    const bool w3 = wave < 6;                                   // waves rf = 0 also carry the third row fragment where 68 rows are needed

    // ================= End^T: d skip = (d(m, logs) W_end^T) * mask on the 68 tile rows =================
    TLS();
    zero_acc();
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
        const unsigned char* slot = begin_step(IC<0>{});
        mma192(slot, DT + (2 * j) * (WN_XR * 64), DT + (2 * j + 1) * (WN_XR * 64), w3, 0);
        end_step();
    }
    TLS();
    {
        const int ln = fresh_lane(), l15x = ln & 15, lqx = ln >> 4;
        const int rb = rf * 32 + 4 * lqx;
        unsigned char* const dc = DS + cf * (WN_XR * 64);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int to = tile_off_of(l15x, lqx, h, 0);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = rb + 16 * rt + i;
                    *reinterpret_cast<unsigned short*>(dc + row * 64 + to) = bf16_bits(acc[rt][h][i] * MK[row]);
                }
            if (w3 && lqx == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<unsigned short*>(dc + (64 + i) * 64 + to) = bf16_bits(a3[h][i] * MK[64 + i]);
            }
        }
    }

    const uint32_t thr = drop_threshold(p.drop_p);
    const float ik = drop_inv_keep(thr);
    uint32_t seed0 = p.seed;
    if (DROP && p.seed_ptr) seed0 += *p.seed_ptr;
    const uint32_t lds0 = lds_addr(wb_smem);

    // ================= one layer (LAST: the last layer of the network, the first one here) =================
    auto layer = [&](auto LAST_, const int l) __attribute__((always_inline)) {
        constexpr bool last = decltype(LAST_)::value;
        TLS();
        // ---- the layer's kept gates (t, s), prefetched: 16 (+ 8: tile rows 64..67 of the last layer; every wave issues them, the count below is uniform)
        // loads per lane that return under the RS^T GEMM instead of in front of the gate derivative ----
        constexpr int roff = last ? 0 : WN_PAD;                 // tile row of accumulator row 0
        constexpr int NG = last ? 24 : 16;
        uint32_t gw[2][2][4], gw3[2][4];
        {
            const int ln = fresh_lane(), l15x = ln & 15, lqx = ln >> 4;
            const Rsrc rg = mk_rsrc(pick4(p.gates, l), (long)p.rows * (2 * WN_H * 2));
            const int g0 = xr0 + roff + rf * 32 + 4 * lqx;      // global row of accumulator row 0
            const uint32_t cb = (uint32_t)(cf * 32 + l15x) * 4u;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {                   // (rows outside the tensor: clamped garbage is fine, those rows are never stored or valid)
                    int g = g0 + 16 * rt + i;
                    g = g < 0 ? 0 : (g >= p.rows ? p.rows - 1 : g);
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        gw[rt][h][i] = (ABL & 8) ? 0x3f003e80u + (uint32_t)i : __builtin_amdgcn_raw_buffer_load_b32(rg, (uint32_t)(g * (2 * WN_H * 2)) + cb + 64u * h, 0, 0);
                }
            if constexpr (last) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    int g = g0 + 64 + i;                        // (waves rf = 0: tile row 64 + i + 4 lq; lanes lq > 0 and waves rf = 1: rows that do not exist in the tile, never used)
                    g = g < 0 ? 0 : (g >= p.rows ? p.rows - 1 : g);
#pragma unroll
                    for (int h = 0; h < 2; ++h)
                        gw3[h][i] = (ABL & 8) ? 0x3f003e80u : __builtin_amdgcn_raw_buffer_load_b32(rg, (uint32_t)(g * (2 * WN_H * 2)) + cb + 64u * h, 0, 0);
                }
            }
        }
        constexpr int NGX = (ABL & 8) ? 0 : NG;
        // ---- RS_l^T: d acts = [d x_{l+1} | d skip] W^T.  Last layer: d skip only, on all 68 tile rows; else on the 64 window rows.
        // Behind slab 0's DMAs: the NG gate loads; behind slab 1's: those and the copy-out's stores; from slab 2 on all of them are older ----
        zero_acc();
        if constexpr (last) {
            StaticFor<3>::run([&](auto J_) __attribute__((always_inline)) {
                constexpr int j = decltype(J_)::value;
                const unsigned char* slot = begin_step(IC<(j == 0 ? NGX : (j == 1 ? NGX + ((ABL & 4) ? 0 : XC) : 0))>{});
                if constexpr (j == 0) copy_out(DS, WN_XR, halo + WN_PAD, p.dskip, WN_H * 2, 64, 0);            // d skip (kept: DY of the Res_Skip weight gradients)
                mma192(slot, DS + (2 * j) * (WN_XR * 64), DS + (2 * j + 1) * (WN_XR * 64), w3, 0);
                end_step();
            });
        } else {
            StaticFor<3>::run([&](auto J_) __attribute__((always_inline)) {      // K chunks 0..5: d x_{l+1} (window rows)
                constexpr int j = decltype(J_)::value;
                const unsigned char* slot = begin_step(IC<(j == 0 ? NGX : (j == 1 ? NGX + ((ABL & 4) ? 0 : XC) : 0))>{});
                if constexpr (j == 0) copy_out(DX, WN_WIN, halo, pick4(p.dh, l + 1), WN_H * 2, 64, 0);           // d x_{l+1} (kept: DY of the Res_Skip weight gradient)
                mma192(slot, DX + (2 * j) * (WN_WIN * 64), DX + (2 * j + 1) * (WN_WIN * 64), false, 0);
                end_step();
            });
#pragma unroll 1
            for (int j = 0; j < 3; ++j) {                       // K chunks 6..11: d skip (window row r = tile row r + 2)
                const unsigned char* slot = begin_step(IC<0>{});
                mma192(slot, DS + (2 * j) * (WN_XR * 64), DS + (2 * j + 1) * (WN_XR * 64), false, WN_PAD);
                end_step();
            }
        }
        // ---- gate derivative (autograd of Modules.py:885-887 and of the dropout at :862): (da, ds) kept packed as bf16 pairs ----
        TLS();
        // The tanh-side gradients da go straight into the tile DT (tile rows roff ..: its last readers - End^T / the previous layer's exchange - are at least
        // three slab barriers back), the sigmoid-side ds wait in registers as bf16 pairs (rows i, i + 1) until the second K pass rewrites the tile.
        uint32_t pkd[2][2][2];                                  // [rt][h][i >> 1]
        {
            const int ln = fresh_lane(), l15x = ln & 15, lqx = ln >> 4;
            const int rb = rf * 32 + 4 * lqx;
            const int jch0 = cf * 32 + l15x;                    // (shadows the kernel-wide one)
            const int g0 = xr0 + roff + rb;                     // global row of accumulator row 0
            const uint32_t rk0 = (uint32_t)g0 * 0x9E3779B1u + seed0 + (uint32_t)l;      // drop_rowkey(seed + l, row) = fmix_head(row * M + seed + l)
            auto rowkey = [&](int c) __attribute__((always_inline)) -> uint32_t { return fmix_head(rk0 + (uint32_t)c * 0x9E3779B1u); };
            // owned TILE rows [own_lo, own_hi): the conditioning gradient sums them per utterance
            const int own_lo = halo + WN_PAD, own_hi = own_lo + lim;
            const bool one_utt = COND && lim > 0 && UT[own_lo] == UT[own_lo + lim - 1];       // (wave-uniform) the rule: an utterance is hundreds of rows
            long long* const dcl = COND ? reinterpret_cast<long long*>(p.dcond) + (long)l * (2 * WN_H) + jch0 : nullptr;     // (fixed-point accumulators: device_common.h)
            unsigned char* const dc = DT + cf * (WN_XR * 64) + (rb + roff) * 64;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t jkey = drop_colkey((uint32_t)(jch0 + 16 * h));
                const int to0 = tile_off_of(l15x, lqx, h, 0), to1 = tile_off_of(l15x, lqx, h, 1);
                float sa = 0.f, ss = 0.f;
                int cur_u = -1;
                // c: accumulator row (tile row roff + rb + c) -> da (returned), ds
                auto gate = [&](float d, uint32_t w, int c, float& ds) __attribute__((always_inline)) -> float {
                    const float t = __uint_as_float(w << 16), sg = __uint_as_float(w & 0xFFFF0000u);
                    const float dsg = d * sg;
                    float da = dsg * (1.f - t * t);
                    ds = dsg * t * (1.f - sg);
                    if constexpr (COND) {
                        const int tr = roff + rb + c;
                        const bool own = tr >= own_lo && tr < own_hi;
                        if (one_utt) { sa += own ? da : 0.f; ss += own ? ds : 0.f; }
                        else if (own) {                         // windows that straddle utterances: this lane's own runs, one pair of atomics per run
                            const int u = UT[tr];
                            if (u != cur_u) {
                                if (cur_u >= 0) { long long* dst = dcl + 16 * h + (long)cur_u * p.ldcond; fx_atomic_add(dst, sa); fx_atomic_add(dst + WN_H, ss); }
                                sa = ss = 0.f;
                                cur_u = u;
                            }
                            sa += da; ss += ds;
                        }
                    }
                    if constexpr (DROP) {
                        const uint32_t dd = drop_draw(rowkey(c), jkey);
                        da *= drop_keep_lo(dd, thr, ik); ds *= drop_keep_hi(dd, thr, ik);
                    }
                    return da;
                };
                if constexpr (last) {
                    if (w3) {                                   // tile rows 64..67 (lanes lq = 0; the other lanes' values are never stored): da -> the tile,
#pragma unroll                                                  // ds -> parked in P3 until the second pass
                        for (int i = 0; i < 4; ++i) {
                            float ds;
                            const float da = gate(a3[h][i], gw3[h][i], lqx == 0 ? 64 + i - rb : 1 << 20, ds);
                            if (lqx == 0) {
                                *reinterpret_cast<unsigned short*>(DT + cf * (WN_XR * 64) + (64 + i) * 64 + to0) = bf16_bits(da);
                                *reinterpret_cast<unsigned short*>(wb_smem + BOFF_P3 + cf * 256 + i * 64 + to0) = bf16_bits(ds);
                            }
                        }
                    }
                }
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int i2 = 0; i2 < 2; ++i2) {
                        float ds0, ds1;
                        const float da0 = gate(acc[rt][h][2 * i2], gw[rt][h][2 * i2], 16 * rt + 2 * i2, ds0);
                        const float da1 = gate(acc[rt][h][2 * i2 + 1], gw[rt][h][2 * i2 + 1], 16 * rt + 2 * i2 + 1, ds1);
                        // rows i = 2 i2, 2 i2 + 1 of this 4-row group: the swizzle parity flips where (i + roff) crosses 4 (roff = 2: for i2 = 1)
                        const int to = ((2 * i2 + roff) >> 2) ? to1 : to0;
                        *reinterpret_cast<unsigned short*>(dc + (16 * rt + 2 * i2) * 64 + to) = bf16_bits(da0);
                        *reinterpret_cast<unsigned short*>(dc + (16 * rt + 2 * i2 + 1) * 64 + to) = bf16_bits(da1);
                        pkd[rt][h][i2] = pack_bf16x2(ds0, ds1);
                    }
                if constexpr (COND) {
                    if (one_utt) {                              // the four lanes (lq) of a column hold rows 4 apart: one sum, one pair of atomics
                        sa += __shfl_xor(sa, 16, 64); ss += __shfl_xor(ss, 16, 64);
                        sa += __shfl_xor(sa, 32, 64); ss += __shfl_xor(ss, 32, 64);
                        if (lqx == 0) { long long* dst = dcl + 16 * h + (long)UT[own_lo] * p.ldcond; fx_atomic_add(dst, sa); fx_atomic_add(dst + WN_H, ss); }
                    } else if (cur_u >= 0) {
                        long long* dst = dcl + 16 * h + (long)cur_u * p.ldcond;
                        fx_atomic_add(dst, sa); fx_atomic_add(dst + WN_H, ss);
                    }
                }
            }
        }
        TLS();
        // the sigmoid-side half -> DT at the pass boundary
        auto write_ds_half = [&]() __attribute__((always_inline)) {
            const int ln = fresh_lane(), l15x = ln & 15, lqx = ln >> 4;
            const int rb = rf * 32 + 4 * lqx;
            unsigned char* const dc = DT + cf * (WN_XR * 64) + (rb + roff) * 64;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int to0 = tile_off_of(l15x, lqx, h, 0), to1 = tile_off_of(l15x, lqx, h, 1);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int i2 = 0; i2 < 2; ++i2) {
                        const uint32_t w = pkd[rt][h][i2];
                        const int to = ((2 * i2 + roff) >> 2) ? to1 : to0;
                        *reinterpret_cast<unsigned short*>(dc + (16 * rt + 2 * i2) * 64 + to) = (unsigned short)(w & 0xFFFFu);
                        *reinterpret_cast<unsigned short*>(dc + (16 * rt + 2 * i2 + 1) * 64 + to) = (unsigned short)(w >> 16);
                    }
                if constexpr (last) {
                    if (w3 && lqx == 0) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            *reinterpret_cast<unsigned short*>(DT + cf * (WN_XR * 64) + (64 + i) * 64 + to0) = *reinterpret_cast<const unsigned short*>(wb_smem + BOFF_P3 + cf * 256 + i * 64 + to0);
                    }
                }
            }
        };

        // ---- In_l^T: two K passes (da, ds) x 5 taps x 3 slabs; wave (rf, cp, kh) multiplies chunk kh of every slab over 32 rows x 64 columns.
        // Software pipeline as in the forward: step n reads slab n's fragments into register set n & 1 and multiplies slab n - 1 from the other set ----
        zero_acc();
        {
            Chunk16 fa[2][2], fb[2][4];                        // [set][rt], [set][ct]
            auto mma = [&](auto SET_) __attribute__((always_inline)) {
                constexpr int st = decltype(SET_)::value;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = mfma16_bf16<!(ABL & 2)>(fa[st][rt], fb[st][ct], acc[rt][ct]);
            };
            const int lnI = fresh_lane(), l15i = lnI & 15, lqi = lnI >> 4;
            const uint32_t dtk = lds0 + (uint32_t)(BOFF_DT + kh * (WN_XR * 64));       // this wave's K chunk of a slab's two: tile chunk 2 jj + kh
            const uint32_t sbk = (uint32_t)(kh * 12288 + cp * 4096 + swz16(l15i, lqi));
            uint32_t ao0 = 0, ao1 = 0;
            auto step = [&](auto N_) __attribute__((always_inline)) {
                constexpr int n = decltype(N_)::value;
                constexpr int m = n >= 15 ? n - 15 : n, t = m / 3, jj = m - 3 * t, st = n & 1;
                const unsigned char* slot = begin_step(IC<((n == 1 || n == 16) && !(ABL & 4) ? XC : 0)>{});
                if constexpr (n == 0) copy_out(DT, WN_XR, halo + WN_PAD, pick4(p.dins, l), (int)p.ldin * 2, 128, 0);        // da half of dins_l
                if constexpr (n == 15) TLS();
                if constexpr (n == 15) {                        // second pass: the tile is rewritten with the sigmoid-side half (every read of it has landed: lgkmcnt(0) + barrier above)
                    write_ds_half();
                    plain_barrier();
                    copy_out(DT, WN_XR, halo + WN_PAD, pick4(p.dins, l), (int)p.ldin * 2, 128, 64);                         // ds half
                }
                if constexpr (jj == 0) {                        // this tap's rows of the tile: row + t, swizzled
                    ao0 = dtk + (uint32_t)swz16(rf * 32 + l15i + t, lqi);
                    ao1 = dtk + (uint32_t)swz16(rf * 32 + 16 + l15i + t, lqi);
                }
                const uint32_t sa = lds_addr(slot) + sbk;
                fa[st][0] = lds16_asm<2 * jj * (WN_XR * 64)>(ao0);
                fa[st][1] = lds16_asm<2 * jj * (WN_XR * 64)>(ao1);
                fb[st][0] = lds16_asm<0>(sa); fb[st][1] = lds16_asm<1024>(sa); fb[st][2] = lds16_asm<2048>(sa); fb[st][3] = lds16_asm<3072>(sa);
                if constexpr (n > 0) { lgkm_wait<6>(fa[st ^ 1], fb[st ^ 1]); mma(IC<st ^ 1>{}); }
                __builtin_amdgcn_sched_barrier(0);
                end_step();
            };
            StaticFor<30>::run([&](auto J_) __attribute__((always_inline)) { step(J_); });
            lgkm_wait<0>(fa[1], fb[1]);
            mma(IC<1>{});                                       // slab 29
        }
        // ---- partners swap halves of their partial sums: the wave keeps fragments ct = 2 kh, 2 kh + 1 (columns 64 cp + 32 kh ..: its cf-th
        // 32-channel block) and hands the other two to wave ^ 1.  One round: 8 registers through the tile, 8 through the ring slot of the slab just used ----
        TLS();
        f32x4 fin[2][2];                                        // [rt][h]: rows 32 rf + 16 rt + 4 lq + i, channel 32 cf + 16 h + l15
        {
            const int lane = fresh_lane();                      // (shadows the kernel-wide one)
            float* const xs0 = reinterpret_cast<float*>(DT);
            float* const xs1 = reinterpret_cast<float*>(wb_smem + BOFF_RING + ((snext + BW_NS - 1) % BW_NS) * WN_SLAB);      // slot of slab snext - 1
            if constexpr (!(ABL & 16)) {
                plain_barrier();                                // every wave is done reading the tile and the last slab
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        xs0[(wave * 8 + h * 4 + i) * 64 + lane] = kh ? acc[0][h][i] : acc[0][2 + h][i];
                        xs1[(wave * 8 + h * 4 + i) * 64 + lane] = kh ? acc[1][h][i] : acc[1][2 + h][i];
                    }
                plain_barrier();
            }
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float o0 = (ABL & 16) ? 0.f : xs0[((wave ^ 1) * 8 + h * 4 + i) * 64 + lane];
                    const float o1 = (ABL & 16) ? 0.f : xs1[((wave ^ 1) * 8 + h * 4 + i) * 64 + lane];
                    fin[0][h][i] = (kh ? acc[0][2 + h][i] : acc[0][h][i]) + o0;
                    fin[1][h][i] = (kh ? acc[1][2 + h][i] : acc[1][h][i]) + o1;
                }
        }
        TLS();
        // ---- d x_l = (conv^T + d x_{l+1}) * mask -> DX (bf16, in place); l = 0: fp32 rows for the Start conv's weight gradient ----
        {
            const int ln = fresh_lane(), l15x = ln & 15, lqx = ln >> 4;
            const int rb = rf * 32 + 4 * lqx;
            const int jch0 = cf * 32 + l15x;
            unsigned char* const xc = DX + cf * (WN_WIN * 64) + rb * 64;
            const float* const mk = MK + rb + WN_PAD;
            const bool fp32_rows = l == 0 && !p.dh0_bf16;      // (wave-uniform)
            const Rsrc r0 = mk_rsrc(p.dh[0], fp32_rows ? (long)p.rows * (WN_H * 4) : 0);
            const uint32_t own0 = (uint32_t)(rb - halo);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int to = tile_off_of(l15x, lqx, h, 0);
                const uint32_t v00 = (uint32_t)((t0 + rb) * (WN_H * 4) + (jch0 + 16 * h) * 4);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = 16 * rt + i;
                        unsigned short* xp = reinterpret_cast<unsigned short*>(xc + c * 64 + to);
                        const float xin = last ? 0.f : __uint_as_float((uint32_t)*xp << 16);
                        const float v = (fin[rt][h][i] + xin) * mk[c];
                        *xp = bf16_bits(v);
                        const bool ok = own0 + (uint32_t)c < (uint32_t)lim;
                        // (l = 0 is followed by Start^T, whose steps wait conservatively: these stores are in no exact count)
                        if constexpr (!(ABL & 4)) { if (fp32_rows) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r0, ok ? v00 + (uint32_t)(c * (WN_H * 4)) : OOB, 0, 0); }
                    }
            }
        }
    };
#pragma unroll 1
    for (int l = L - 1; l >= 0; --l) {
        if (l == L - 1) layer(IC<1>{}, l); else layer(IC<0>{}, l);
    }

    TLS();
    // ================= Start^T: d x_a += d x_0 W_start^T (K = 192, 96 columns of a 128-column image: 2 slabs of 3 chunks); the ring drains =================
    zero_acc();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if (j == 0) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const unsigned char* slot = wb_smem + BOFF_RING + (snext % BW_NS) * WN_SLAB;
        ++snext;
        // d x_0 as bf16 rows (DY of the Start conv's weight gradient): the finished tile, 16 bytes per store, behind the step's barrier
        // (j = 1's vmcnt(0) also waits for these two stores: the last step)
        if (j == 0 && p.dh0_bf16) copy_out(DX, WN_WIN, halo, p.dh[0], WN_H * 2, 64, 0);
        if (cf < 3) {
            Chunk16 fa[3][2], fb[3][2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) fa[c][rt] = lds16(DX + (3 * j + c) * (WN_WIN * 64) + offA + rt * 1024 + bl);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) fb[c][ct] = lds16(slot + c * 8192 + cf * 2048 + ct * 1024 + bl);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = mfma16_bf16<!(ABL & 2)>(fa[c][rt], fb[c][ct], acc[rt][ct]);
        }
    }
    TLS();
    if (cf < 3) {
        int rb = rbw;
        asm volatile("" : "+v"(rb));
        const Rsrc rx = mk_rsrc(p.dx, (long)p.rows * p.lddx * 4);
        const uint32_t own0 = (uint32_t)(rb - halo);
        float old[2][2][4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool cok = jch0 + 16 * h < p.C2;
            const uint32_t vx0 = (uint32_t)((t0 + rb) * (int)p.lddx + jch0 + 16 * h) * 4u;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = 16 * rt + i;
                    const bool ok = cok && own0 + (uint32_t)c < (uint32_t)lim;
                    old[h][rt][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, ok ? vx0 + (uint32_t)(c * (int)p.lddx * 4) : OOB, 0, 0));
                }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool cok = jch0 + 16 * h < p.C2;
            const uint32_t vx0 = (uint32_t)((t0 + rb) * (int)p.lddx + jch0 + 16 * h) * 4u;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = 16 * rt + i;
                    const bool ok = cok && own0 + (uint32_t)c < (uint32_t)lim;
                    if constexpr (!(ABL & 4)) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(old[h][rt][i] + acc[rt][h][i]), rx, ok ? vx0 + (uint32_t)(c * (int)p.lddx * 4) : OOB, 0, 0);
                }
        }
    }
    TLS();
}

template <bool DROP, bool COND, int ABL = 0>
int launch_wn_bwd(const wn_bwd_args& k, dim3 grid, hipStream_t s)
{
#ifdef GLOWTTS_TOOLS
    if constexpr (ABL == 0 && DROP && !COND) {
        switch (GLOWTTS_TUNABLE("GLOWTTS_WN_BWD_ABL", 0)) {
            case 1: return launch_wn_bwd<DROP, COND, 1>(k, grid, s);
            case 2: return launch_wn_bwd<DROP, COND, 2>(k, grid, s);
            case 3: return launch_wn_bwd<DROP, COND, 3>(k, grid, s);
            case 4: return launch_wn_bwd<DROP, COND, 4>(k, grid, s);
            case 8: return launch_wn_bwd<DROP, COND, 8>(k, grid, s);
            case 12: return launch_wn_bwd<DROP, COND, 12>(k, grid, s);
            case 13: return launch_wn_bwd<DROP, COND, 13>(k, grid, s);
            case 14: return launch_wn_bwd<DROP, COND, 14>(k, grid, s);
            case 16: return launch_wn_bwd<DROP, COND, 16>(k, grid, s);
            case 64: return launch_wn_bwd<DROP, COND, 64>(k, grid, s);
            case 29: return launch_wn_bwd<DROP, COND, 29>(k, grid, s);
            case 31: return launch_wn_bwd<DROP, COND, 31>(k, grid, s);
            default: break;
        }
    }
#endif
    if constexpr (ABL == 0 && DROP && !COND) {                  // (test hook: the unconditioned training shape with conservative waits)
        if (glowtts_wavenet_safe_waits_flag()) return launch_wn_bwd<DROP, COND, 128>(k, grid, s);
    }
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wn_bwd_kernel<DROP, COND, ABL>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return GLOWTTS_E_LAUNCH;
        attr_done = true;
    }
    GLOWTTS_NOTE_STATIC("wn_bwd<%s%s>", DROP ? "drop" : "nodrop", COND ? ",cond" : "");
    hipLaunchKernelGGL((wn_bwd_kernel<DROP, COND, ABL>), grid, dim3(WN_NT), BW_LDS, s, k);
    RET_LAUNCH();
}

}  // namespace

// the transposed images of F flows (see glowtts_wavenet_pack_images in include/glowtts_hip.h), in the order the backward consumes them
int glowtts_wavenet_pack_bwd_images(const float* w_start, const float* w_in, const float* w_rs, const float* w_rs_last, const float* w_end,
                                    int F, int L, int C2, void* img_bwd, void* stream)
{
    const int H = WN_H;
    const int64_t S = WN_SLAB, stride = (int64_t)(36 * L + 2) * S;
    unsigned char* img = static_cast<unsigned char*>(img_bwd);
    // [End^T 3][layer L-1: RS^T 3, In^T da 15, In^T ds 15][layer l < L-1: RS^T 6, da 15, ds 15 ...][Start^T 2]; In^T da of layer l starts at
    // slab 42 + 36 (L - 2 - l) for every l (6 for the last layer), RS^T of layer l < L - 1 six slabs before it
    int rc = glowtts_pack_weight_strided(w_end, F, 1, 2 * C2, H, 1, 1, GLOWTTS_PERM_PAIR, C2, GLOWTTS_BF16, img, stride, 0, 0, stream);
    if (rc == GLOWTTS_OK) rc = glowtts_pack_weight_strided(w_rs_last, F, 1, H, H, 1, 1, GLOWTTS_PERM_NONE, 0, GLOWTTS_BF16, img + 3 * S, stride, 0, 0, stream);
    if (rc == GLOWTTS_OK && L > 1)
        rc = glowtts_pack_weight_strided(w_rs, F * (L - 1), L - 1, 2 * H, H, 1, 1, GLOWTTS_PERM_NONE, 0, GLOWTTS_BF16, img + (36 + 36 * (int64_t)(L - 2)) * S, stride, -36 * S, 0, stream);
    for (int half = 0; half < 2 && rc == GLOWTTS_OK; ++half)
        rc = glowtts_pack_weight_strided(w_in + (int64_t)half * H * H * WN_TAPS, F * L, L, H, H, WN_TAPS, 1, GLOWTTS_PERM_NONE, 0, GLOWTTS_BF16,
                                         img + (42 + 36 * (int64_t)(L - 2) + 15 * half) * S, stride, -36 * S, (int64_t)2 * H * H * WN_TAPS, stream);
    if (rc == GLOWTTS_OK) rc = glowtts_pack_weight_strided(w_start, F, 1, H, C2, 1, 1, GLOWTTS_PERM_NONE, 0, GLOWTTS_BF16, img + 36 * (int64_t)L * S, stride, 0, 0, stream);
    return rc;
}

extern "C" int glowtts_wavenet_bwd(const glowtts_flow_dims* d, const glowtts_flow_params* p, const glowtts_flow_acts* a, const glowtts_flow_grads* g,
                                   void* stream)
{
    if (!d || !p || !a || !g || !p->wn_img_t || !a->rowmask || !g->dx || !g->douts_bf || !g->dskip) return GLOWTTS_E_ARG;
    const int C2 = d->C / 2;
    if (d->precision != GLOWTTS_BF16 || !d->act_bf16 || d->H != WN_H || d->ksize != WN_TAPS || d->L < 1 || d->L > WN_MAXL ||
        (d->C & 7) || C2 <= 64 || C2 > 96 || p->end.npad != 192 || p->in[0].npad != 2 * WN_H) return GLOWTTS_E_ARG;
    // inline weight gradients and the GR-mode per-row (pitch) conditioning gradient: per-conv path only
    if (!g->defer_wgrad || g->pitch_rows || p->cond_rows) return GLOWTTS_E_ARG;
    const bool cnd = g->dcond && p->cond;
    if (cnd && (int64_t)d->B * p->ldcond * 4 >= ((int64_t)1 << 31)) return GLOWTTS_E_ARG;
    const int Tp = d->T + 2 * GLOWTTS_ROW_PAD;
    const int64_t R = (int64_t)d->B * Tp;
    if (R * 2 * WN_H * 2 >= ((int64_t)1 << 31) || R * d->C * 4 >= ((int64_t)1 << 31)) return GLOWTTS_E_ARG;
    wn_bwd_args k;
    memset(&k, 0, sizeof(k));
    k.rows = (int)R; k.rows_per_utt = Tp; k.L = d->L; k.C2 = C2;
    k.wimg = static_cast<const unsigned char*>(p->wn_img_t);
    k.douts_bf = g->douts_bf; k.ldo = p->end.npad; k.rowmask = a->rowmask;
    k.drop_p = d->drop_p; k.seed = d->seed; k.seed_ptr = d->seed_ptr;
    k.dskip = g->dskip; k.ldin = p->in[0].npad; k.dx = g->dx; k.lddx = d->C;
    for (int l = 0; l < d->L; ++l) {
        if (!a->gates[l] || !g->dins[l] || !g->dh[l]) return GLOWTTS_E_ARG;
        k.gates[l] = a->gates[l]; k.dins[l] = g->dins[l]; k.dh[l] = g->dh[l];
        k.dh0_bf16 = g->dh0_bf16;
    }
    const int nvalid = WN_WIN - 2 * WN_PAD * (d->L - 1);
    const dim3 grid((unsigned)((R + nvalid - 1) / nvalid));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (cnd) { k.dcond = reinterpret_cast<float*>(g->dcond); k.ldcond = p->ldcond; }
#ifdef GLOWTTS_TOOLS
    k.stagger = GLOWTTS_TUNABLE("GLOWTTS_WN_STAGGER", 0);
    if (!cnd && (GLOWTTS_TUNABLE("GLOWTTS_WN_BWD_ABL", 0) & 64)) k.tl = reinterpret_cast<long long*>(g->dcond);      // tools/bench_wn.py passes the stamp buffer here
#endif
    if (d->drop_p > 0.f) return cnd ? launch_wn_bwd<true, true>(k, grid, s) : launch_wn_bwd<true, false>(k, grid, s);
    return cnd ? launch_wn_bwd<false, true>(k, grid, s) : launch_wn_bwd<false, false>(k, grid, s);
}
