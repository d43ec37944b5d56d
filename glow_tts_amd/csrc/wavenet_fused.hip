// Fused coupling network of one decoder flow for gfx950: Start conv -> L x [In_l (k = 5) + dropout + conditioning + tanh * sigmoid ->
// Res_Skip_l + residual / skip] -> End conv + affine coupling (Modules.py:785-806, 858-887) in ONE launch.
//
// Why (round-2 profile): as ten launches per flow the chain sat at 0.12 of the MFMA peak - every kernel is a fetch
// burst, a short K loop and a store burst that overlap with nothing, and B = 32 leaves 12 928 rows, ~50 per CU.  Here one persistent
// workgroup per CU owns a row tile through the whole network:
//   * 12 waves (3 per SIMD).  A 64-row compute window per workgroup; the k = 5 taps make the valid region shrink by 2 rows per layer on each
//     side, so the window yields 64 - 4 (L - 1) = 52 valid output rows for L = 4 (recomputed halo: 1.23 x the MFMA work, 249 workgroups at
//     B = 32: one round on 256 CUs).  The WaveNet state x_l lives in LDS as bf16 ([6 K chunks][68 rows][64 B], swizzled like every MFMA
//     A tile of this library), tanh * sigmoid likewise; the skip sum stays in accumulator registers across the layers.
//   * ALL weights of the flow are one pre-packed image of 24 KiB slabs ([384 n][64 B] = one (tap, K chunk) of In_l, one K chunk of
//     Res_Skip_l, two K chunks of the 192-column convs), streamed in order through a 4-slot LDS ring by LDS-DMA (global_load_lds_dwordx4,
//     source-side swizzle), two 1-KiB units per wave and slab: one counted s_waitcnt vmcnt + one raw s_barrier per slab, two slabs in
//     flight while one is multiplied.  Per slab every wave issues 4 x v_mfma_f32_32x32x16_bf16 (32 rows x 64 columns x 32 k).
//     Every CU reads every weight byte (3.5 MB per flow and CU from L2): at ~50 rows per CU this path is co-bound by the matrix pipes and
//     by L2 -> LDS bandwidth (64 flop per weight byte), which is why the tile is not smaller than 64 rows.
//   * kept activations (training) leave through the epilogues: gate pairs straight from registers, x_l / tanh * sigmoid as 16-byte
//     pieces copied out of their LDS tiles while the next GEMM runs.
// Arithmetic is the unfused path's (same bf16 roundings of x_l, gates, acts, same dropout hash): results differ only by fp32
// accumulation order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/glowtts_hip.h"
#include "tunable.h"
#include "launch_log.h"
#include "wavenet_common.h"
#include "actnorm_math.h"

namespace {

// LDS map (bytes)
constexpr int OFF_XT = 0;                                       // x_l: [6][68][64]; after the last layer: bf16 skip sum [6][64][64]
constexpr int SZ_XT = WN_KCH * WN_XR * 64;
constexpr int OFF_AT = OFF_XT + SZ_XT;                          // tanh * sigmoid: [6][64][64]; before layer 0: x_a [3][96][64]
constexpr int SZ_AT = WN_KCH * WN_WIN * 64;
constexpr int OFF_RING = OFF_AT + SZ_AT;
constexpr int OFF_BT = OFF_RING + WN_NS * WN_SLAB;              // biases (floats)
constexpr int BT_START = 0, BT_IN = 192, BT_RS = BT_IN + WN_MAXL * 384, BT_RSL = BT_RS + (WN_MAXL - 1) * 384, BT_END = BT_RSL + 192;
constexpr int BT_FLOATS = BT_END + 192;
constexpr int OFF_MK = OFF_BT + BT_FLOATS * 4;                  // rowmask of the 68 state rows
constexpr int OFF_UT = OFF_MK + WN_XR * 4;                      // conditioning row index of the 68 state rows
constexpr int WN_LDS = OFF_UT + WN_XR * 4;
static_assert(WN_LDS <= 160 * 1024, "LDS budget");
static_assert(SZ_AT >= 3 * WN_SROWS * 64, "the Start operand tile aliases the acts tile");

typedef StaticFor<WN_TAPS * WN_KCH> StaticFor30;

struct wn_fwd_args {
    int rows, rows_per_utt, L, C2, reverse, keep, safe_waits;
    const float* xsrc; int64_t ldx;               // [rows][ldx]: channels [0, C2) = x_a, [C2, 2 C2) = x_b
    float* xdst; int64_t ldxd;                    // x_b' -> xdst[r][C2 + j]
    const float* rowmask;
    const unsigned char* wimg;
    const float* b_start; const float* b_in[WN_MAXL]; const float* b_rs[WN_MAXL]; const float* b_end;
    const float* cond; int64_t ldcond; int cond_rows;
    float drop_p; uint32_t seed; const uint32_t* seed_ptr;
    void* hs[WN_MAXL]; void* gates[WN_MAXL]; void* acts[WN_MAXL];       // kept (bf16)
    float* skip; float* outs; int64_t ldo;                              // kept (fp32)
    void* skip_bf;                                                      // kept (bf16 copy of skip, [rows][192]; may be null)
    long long* tl;                                                      // tools builds (ABL & 16): per-workgroup phase stamps [grid][32]
    int stagger;                                                        // experiment (tools builds): start delay of workgroup b = ((b >> 3) & 7) * stagger * 512 clocks
    // the NEXT flow's ActNorm + invertible 1x1 conv, applied by the coupling epilogue to the rows it produces (nx_xmid null: not asked for)
    const float* nx_logs; const float* nx_bias; const float* nx_winfo;
    float* nx_xmid; float* nx_xout; uint32_t* nx_xa_bf;
};

// DROP / COND: training-mode dropout / conditioning present (compile-time, so that the unrolled gate epilogue is straight-line code)
// ABL (tools builds only, tools/bench_wn.py): timing ablations - 1: no weight DMAs after the prologue, 2: no MFMAs, 4: no kept-activation stores,
// 16: per-workgroup phase stamps
//
// Round 4: every product runs on v_mfma_f32_16x16x32_bf16 (a wave tile of 32 rows x 64 columns = 2 x 4 fragments, one K chunk of 32 per
// instruction) instead of v_mfma_f32_32x32x16_bf16.  Measured (tools/wn_lab.hip): while a SIMD issues back-to-back 8-pass
// 32x32x16 MFMAs it issues NO vector-memory instruction - the weight DMAs of its waves wait for gaps in the matrix pipe, weight delivery and
// matrix work add up instead of overlapping (387 ns per slab); the 4-pass 16x16x32 form leaves the slots (302 ns per slab with the same ring,
// barrier and tiling).  Its fragment reads (lane = (row & 15, 16-byte slot lane >> 4)) need another LDS slot swizzle to stay bank-conflict
// free at every tap shift: slot ^ 2 * ((row >> 2) & 1) (`swz16`; the 32x32 layout's (row >> 2) & 3 gives 2-way conflicts here).
// Accumulator element i of fragment (rt, ct) of a wave: row 16 rt + 4 (lane >> 4) + i, column 16 ct + (lane & 15); under the PAIR packing the
// fragments ct and ct + 2 of a lane hold the (tanh, sigmoid) / (residual, skip) / (m, logs) members of the same channel.
// KEEP / SAFE are compile-time as well: a run-time branch inside the slab loops ends a basic block there, and at a block boundary the compiler's
// own s_waitcnt insertion falls back to lgkmcnt(0) - the MFMAs of slab j then wait for the fragment reads of slab j + 1 that were issued right in
// front of them (the software pipeline below silently degenerates; the round-3 kernel had the keep / safe_waits / first-tap tests inside the loop)
template <bool DROP, bool COND, bool KEEP, bool SAFE = false, int ABL = 0>
__global__ __launch_bounds__(WN_NT) void wn_fwd_kernel(const wn_fwd_args p)
{
    extern __shared__ __attribute__((aligned(1024))) unsigned char wn_smem[];
    unsigned char* const XT = wn_smem + OFF_XT;
    unsigned char* const AT = wn_smem + OFF_AT;
    float* const BT = reinterpret_cast<float*>(wn_smem + OFF_BT);
    float* const MK = reinterpret_cast<float*>(wn_smem + OFF_MK);
    int* const UT = reinterpret_cast<int*>(wn_smem + OFF_UT);

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int rf = wave >= 6 ? 1 : 0, pi = wave - rf * 6;      // 32-row half / column group (64 packed columns) of this wave
    const int L = p.L;
    const int halo = WN_PAD * (L - 1);
    const int nvalid = WN_WIN - 2 * halo;                      // valid output rows of the window
    const int v0 = blockIdx.x * nvalid;                        // first valid (owned) row
    const int t0 = v0 - halo;                                  // global row of window row 0
    const int xr0 = t0 - WN_PAD;                               // global row of state-tile row 0
    constexpr bool keep = KEEP && !(ABL & 4);

    // ---- weight stream: slab s -> ring slot s % 4; this wave's two 1-KiB units are rows [32 wave, 32 wave + 32) of the slab.  Lane i of a unit
    // lands in LDS row i >> 2, slot i & 3, and fetches the global slot (i & 3) ^ swizzle(row) (the involution applied on the source side) ----
    const int lrow = lane >> 2, qa = (lane & 3) ^ (((lane >> 4) & 1) << 1);
    const unsigned char* const wsrc = p.wimg + (uint32_t)((wave * 32 + lrow) * 64 + qa * 16);
    auto issue = [&](int s) __attribute__((always_inline)) {
        const unsigned char* src = wsrc + (size_t)s * WN_SLAB;
        unsigned char* dst = wn_smem + OFF_RING + (s & (WN_NS - 1)) * WN_SLAB + wave * 2048;
#pragma unroll
        for (int u = 0; u < 2; ++u)
            __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(src + u * 1024), (void __attribute__((address_space(3)))*)(dst + u * 1024), 16, 0, 0);
    };
    int snext = 0;                                             // slab being multiplied
    int tli = 0;
    auto TLS = [&]() __attribute__((always_inline)) { if constexpr ((ABL & 16) != 0) { if (tid == 0) p.tl[blockIdx.x * 32 + tli] = (long long)__builtin_readcyclecounter(); ++tli; } };
    TLS();
    // A slab step: begin_step() = this wave's DMAs of slab `snext` have landed (the two slabs behind it may fly: vmcnt(4)), barrier
    // (everyone's have landed, everyone is done with slab snext - 1), -> its ring slot; ... fragment reads, MFMAs ...; end_step() refills
    // the slot the barrier freed with slab snext + 3.  The last three slabs (the End conv) drain the ring: waits 4 / 2 / 0, no refill.
    // X = vector-memory operations this wave has issued BEHIND the DMAs of slab snext besides the two younger slabs' four DMAs: the global
    // stores of the epilogue in front of this GEMM and of the copy-outs.  Memory operations retire in order (vmcnt counts loads and stores
    // alike on gfx9), so vmcnt(4 + X) waits for exactly slab snext; with a smaller count the wave would also wait for its own stores to be
    // acknowledged (measured: ~4 000 clocks at the head of every GEMM).  X must never exceed the real count: every counted operation is an
    // unconditional buffer instruction (invalid rows are dropped through an out-of-range offset, not branched around); `p.safe_waits`
    // (tests) runs the conservative vmcnt(4) everywhere and must give bit-identical results.
    auto begin_step = [&](auto X_) __attribute__((always_inline)) -> const unsigned char* {
        constexpr int X = decltype(X_)::value;
        if constexpr (X == 0 || SAFE) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(4 + X) : "memory");
        return wn_smem + OFF_RING + (snext & (WN_NS - 1)) * WN_SLAB;
    };
    constexpr int XG = 16;                                     // stores of a gate / last Res_Skip epilogue (one per accumulator pair)
    constexpr int XC = 2;                                      // stores of a copy_out
    auto end_step = [&]() __attribute__((always_inline)) {
        if (!(ABL & 1)) issue(snext + WN_NS - 1);
        ++snext;
    };

    // ---- prologue: x_a -> bf16 operand tile of the Start conv, biases, row masks; the first three slabs stream in meanwhile ----
    {
        const int C2 = p.C2, per_row = C2 >> 2;
        unsigned char* const ST = AT;
        // WN_XR rows of at most 96 / 4 = 24 four-channel pieces: three rounds of the workgroup (two cover C2 <= 88 only)
        constexpr int XA_ROUNDS = (WN_XR * 24 + WN_NT - 1) / WN_NT;
        static_assert(XA_ROUNDS * WN_NT >= WN_XR * (96 / 4), "the x_a staging loop covers every state row at the largest C2");
        float4 xv[XA_ROUNDS]; int xi[XA_ROUNDS];
#pragma unroll
        for (int k = 0; k < XA_ROUNDS; ++k) {
            const int idx = tid + k * WN_NT;
            xi[k] = idx < WN_XR * per_row ? idx : -1;
            const int i = idx / per_row, c4 = idx - i * per_row;
            int g = xr0 + i;
            g = g < 0 ? 0 : (g >= p.rows ? p.rows - 1 : g);
            xv[k] = xi[k] >= 0 ? *reinterpret_cast<const float4*>(p.xsrc + (int64_t)g * p.ldx + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // biases -> LDS table (every load is issued before the first use; unrolled over the layers: no dynamic indexing of the arguments)
        {
            const int i = tid;
            if (i < WN_H) { BT[BT_START + i] = p.b_start[i]; BT[BT_RSL + i] = pick4(p.b_rs, L - 1)[i]; BT[BT_END + i] = i < 2 * C2 ? p.b_end[i] : 0.f; }
            if (i < 2 * WN_H) {
#pragma unroll
                for (int l = 0; l < WN_MAXL; ++l) {
                    if (l < L) BT[BT_IN + l * 384 + i] = p.b_in[l][i];
                    if (l < L - 1) BT[BT_RS + l * 384 + i] = p.b_rs[l][i];
                }
            }
        }
        if (tid < WN_XR) {
            int g = xr0 + tid;
            g = g < 0 ? 0 : (g >= p.rows ? p.rows - 1 : g);
            MK[tid] = p.rowmask[g];
            UT[tid] = p.cond_rows ? g : g / p.rows_per_utt;
        }
        issue(0); issue(1); issue(2);
#ifdef GLOWTTS_TOOLS
        for (int k = 0; k < (int)((blockIdx.x >> 3) & 7) * p.stagger; ++k) __builtin_amdgcn_s_sleep(8);
#endif
#pragma unroll
        for (int k = 0; k < XA_ROUNDS; ++k) {
            if (xi[k] < 0) continue;
            const int i = xi[k] / per_row, c4 = xi[k] - i * per_row;
            const int ch = c4 * 4, kc = ch >> 5, cc = ch & 31;
            uint2 o; o.x = pack_bf16x2(xv[k].x, xv[k].y); o.y = pack_bf16x2(xv[k].z, xv[k].w);
            *reinterpret_cast<uint2*>(ST + kc * (WN_SROWS * 64) + swz16(i, cc >> 3) + (cc & 7) * 2) = o;
        }
        const int npad4 = (96 - C2) >> 2;                      // zero the K padding [C2, 96) (the packed weights are zero there; LDS garbage may be NaN)
        for (int idx = tid; idx < WN_XR * npad4; idx += WN_NT) {
            const int i = idx / npad4, ch = C2 + (idx - i * npad4) * 4, kc = ch >> 5, cc = ch & 31;
            *reinterpret_cast<uint2*>(ST + kc * (WN_SROWS * 64) + swz16(i, cc >> 3) + (cc & 7) * 2) = make_uint2(0u, 0u);
        }
    }

    // per-lane fragment offset.  Row n of a slab (or tile) is 64 bytes; lane (l15, lq) reads slot lq of row base + l15.  A block of 16 rows further
    // on is +1024 bytes (the swizzle has period 8 rows), so one lane value + wave-uniform offsets address every fragment
    const int bl = swz16(l15, lq);
    const int offP = pi * 4096;                                // pair kind: fragments ct = 0..3 (+1024 each) of this wave's 64 columns of a 384-row slab
    const int off1 = pi * 2048;                                // one-fragment kind: fragments ct = 0, 1 of this wave's 32 columns of a 192-row half slab
    const int offA = rf * 2048;                                // this wave's 32-row half of a 64-row tile (fragments rt = 0, 1: +1024)
    // 16-byte copy of the valid rows of an LDS tile [6 chunks][trows][64 B] to a bf16 rows tensor [rows][192]
    auto copy_out = [&](const unsigned char* tile, int trows, int row_off, void* dst) __attribute__((always_inline)) {
        if constexpr ((ABL & 32) != 0) return;
        const Rsrc rd = mk_rsrc(dst, dst ? (long)p.rows * (WN_H * 2) : 0);
        int tid_ = tid;
        asm volatile("" : "+v"(tid_));                         // (opaque: keeps this address arithmetic out of the registers that live across the GEMM loops)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int idx = tid_ + k * WN_NT;
            const int r = idx / 24, pc = idx - r * 24;
            const bool ok = r < nvalid && v0 + r < p.rows;
            const Chunk16 v = lds16(tile + (pc >> 2) * (trows * 64) + swz16(row_off + (ok ? r : 0), pc & 3));
            __builtin_amdgcn_raw_buffer_store_b128(v, rd, ok ? (uint32_t)((v0 + r) * (WN_H * 2) + pc * 16) : OOB, 0, 0);
        }
    };

    f32x4 acc[2][4];                                           // [16-row fragment rt][16-column fragment ct]
    f32x4 skp[2][2];                                           // skip sum of channels 32 pi + 16 h + l15: [rt][h]
    auto zero_acc = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int h = 0; h < 2; ++h) skp[rt][h] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Epilogue addressing.  Accumulator element i of fragment (rt, ct) sits in tile row rb + 16 rt + i, rb = 32 rf + 4 lq, channel column
    // 16 ct' + l15 of the wave's 32 channels (ct' = ct & 1).  Its bf16 slot in a swizzled [rows][64 B] tile: row * 64 + ((q ^ sw(row)) << 4) +
    // (l15 & 7) * 2 with q = 2 ct' + (l15 >> 3) and sw(row) = 2 * ((row >> 2) & 1).  With rb a multiple of 4, (row >> 2) & 1 = (lq + carry) & 1
    // where carry = (i + extra) >> 2 for a tile whose rows are shifted by `extra` (the state tile: + WN_PAD): two lane constants per ct'.
    const int rbw = rf * 32 + 4 * lq;                          // first window row of this lane's accumulator rows (rt = 0, i = 0)
    auto tile_off = [&](int h, int cy) __attribute__((always_inline)) -> int {     // byte offset inside a row for channel half h, carry cy
        return ((((2 * h + (l15 >> 3)) ^ (((lq + cy) & 1) << 1)) & 3) << 4) + (l15 & 7) * 2;
    };
    const int lim = (p.rows - v0) < nvalid ? (p.rows - v0) : nvalid;      // owned rows that exist

    TLS();
    // ================= Start conv: x_0 = (W x_a + b) * mask on the 68 state rows (Modules.py:791) =================
    // one-fragment kind: wave (rf, pi) owns state rows [32 rf, 32 rf + 32) x channels [32 pi, 32 pi + 32); the waves rf = 0 also rows 64..79
    // (of which 64..67 exist) as a third 16-row fragment
    {
        f32x4 a3[2];
        zero_acc();
        a3[0] = a3[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned char* slot = begin_step(IC<0>{});
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (j == 1 && c == 1) break;                   // K = 96 = 3 chunks: slab 1 holds one chunk (the rest of it is never multiplied)
                const unsigned char* At = AT + (2 * j + c) * (WN_SROWS * 64);
                Chunk16 fa[3], fb[2];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) fb[ct] = lds16(slot + c * 12288 + off1 + ct * 1024 + bl);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) fa[rt] = lds16(At + offA + rt * 1024 + bl);
                if (wave < 6) fa[2] = lds16(At + 4096 + bl);   // rows 64..79
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = mfma16_bf16<!(ABL & 2)>(fa[rt], fb[ct], acc[rt][ct]);
                if (wave < 6) {
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) a3[ct] = mfma16_bf16<!(ABL & 2)>(fa[2], fb[ct], a3[ct]);
                }
            }
            end_step();
        }
        TLS();
        // x_0 -> state tile (rows 0..67)
        unsigned char* const xc = XT + pi * (WN_XR * 64);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float b = BT[BT_START + pi * 32 + 16 * h + l15];
            const int to = tile_off(h, 0);
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = rbw + 16 * rt + i;
                    *reinterpret_cast<unsigned short*>(xc + row * 64 + to) = bf16_bits((acc[rt][h][i] + b) * MK[row]);
                }
            if (wave < 6 && lq == 0) {                         // rows 64..67 of the third fragment: the lanes lq = 0
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *reinterpret_cast<unsigned short*>(xc + (64 + i) * 64 + to) = bf16_bits((a3[h][i] + b) * MK[64 + i]);
            }
        }
    }

    TLS();
    // dropout / conditioning constants
    const uint32_t thr = drop_threshold(p.drop_p);
    const float ik = drop_inv_keep(thr);
    uint32_t seed0 = p.seed;
    if (DROP && p.seed_ptr) seed0 += *p.seed_ptr;
    const Rsrc rcond = mk_rsrc(p.cond, COND ? (long)(p.cond_rows ? p.rows : p.rows / p.rows_per_utt) * p.ldcond * 4 : 0);
    const int jch0 = pi * 32 + l15;                            // this lane's channels in 192-wide tensors: jch0 and jch0 + 16
    // Per-utterance conditioning and utterances of at least a tile's 68 rows (>= 128 mel frames): the tile holds at most TWO utterances,
    // rows [0, cbnd) of the first and the rest of the second - eight loads per layer, issued under the GEMM's last slab, and a per-row
    // select instead of per-row loads whose round trips the epilogue waited for twice (+6.7 us per launch against the unconditioned kernel).
    const bool two = COND && !p.cond_rows && p.rows_per_utt >= WN_XR;
    int cu_lo = 0, cu_hi = 0, cbnd = WN_XR;
    if (two) {
        cu_lo = UT[0]; cu_hi = UT[WN_XR - 1];
        cbnd = (cu_lo + 1) * p.rows_per_utt - xr0;             // tile row of the second utterance's first row
    }

    // ================= WaveNet layers =================
#pragma unroll 1
    for (int l = 0; l < L; ++l) {
        const bool last = l == L - 1;
        // ---- In_l: k = 5 conv over the state tile, 30 slabs = (tap, K chunk) ----
        zero_acc();
        float cpre[2][2][2] = {{{0.f, 0.f}, {0.f, 0.f}}, {{0.f, 0.f}, {0.f, 0.f}}};      // [utterance of the tile][channel half h][tanh, sigmoid]
        {
            // Software pipeline over the slab steps: the fragments of slab j are read (LDS -> registers) during step j, its MFMAs run during
            // step j + 1 from the other register set (a "read, wait, multiply" step alternates between an LDS burst with idle matrix pipes
            // and an MFMA burst with an idle LDS).  The ring protocol is unchanged: slab j's slot is read only inside step j.
            Chunk16 fa[2][2], fb[2][4];                        // [set][rt], [set][ct]
            auto mma = [&](auto SET_) __attribute__((always_inline)) {
                constexpr int st = decltype(SET_)::value;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = mfma16_bf16<!(ABL & 2)>(fa[st][rt], fb[st][ct], acc[rt][ct]);
            };
            const uint32_t lds0 = lds_addr(wn_smem);
            uint32_t ao0 = 0, ao1 = 0;
            // one slab step: barrier, the fragment reads of this slab into set kc & 1, the MFMAs of the slab before from the other set, the refill.
            // All 30 steps are straight-line code (taps unrolled): nothing in flight crosses a loop back-edge, where the register allocator may
            // place copies of registers whose asm reads have not landed yet.
            auto step = [&](auto KC_, auto T_) __attribute__((always_inline)) {
                constexpr int kc = decltype(KC_)::value, t = decltype(T_)::value;
                constexpr bool first = t == 0;                           // first tap: nothing to multiply at kc = 0, the kept copy of x_l goes out
                // (the epilogue in front of this GEMM issues no global operation; the copy-out sits behind slab 0's wait)
                const unsigned char* slot;
                if constexpr (first && keep && (kc == 1 || kc == 2)) slot = begin_step(IC<XC>{}); else slot = begin_step(IC<0>{});
                if constexpr (first && kc == 0 && keep) copy_out(XT, WN_XR, halo + WN_PAD, pick4(p.hs, l));       // x_l (kept: X of the In_l weight gradient)
                constexpr int st = kc & 1;
                if constexpr (kc == 0) {                                 // this tap's rows of the state tile: row + t, swizzled
                    ao0 = lds0 + (uint32_t)swz16(rf * 32 + l15 + t, lq);
                    ao1 = lds0 + (uint32_t)swz16(rf * 32 + 16 + l15 + t, lq);
                }
                const uint32_t sa = lds_addr(slot) + (uint32_t)(offP + bl);
                fa[st][0] = lds16_asm<OFF_XT + kc * (WN_XR * 64)>(ao0);
                fa[st][1] = lds16_asm<OFF_XT + kc * (WN_XR * 64)>(ao1);
                fb[st][0] = lds16_asm<0>(sa); fb[st][1] = lds16_asm<1024>(sa); fb[st][2] = lds16_asm<2048>(sa); fb[st][3] = lds16_asm<3072>(sa);
                if constexpr (kc > 0 || !first) { lgkm_wait<6>(fa[st ^ 1], fb[st ^ 1]); mma(IC<st ^ 1>{}); }
                __builtin_amdgcn_sched_barrier(0);
                end_step();
            };
            StaticFor30::run([&](auto J_) __attribute__((always_inline)) { constexpr int j = decltype(J_)::value; step(IC<j % WN_KCH>{}, IC<j / WN_KCH>{}); });
            if constexpr (COND) {
                if (two) {
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const uint32_t co = (uint32_t)((u ? cu_hi : cu_lo) * (int)p.ldcond + l * 2 * WN_H + jch0 + 16 * h) * 4u;
                            cpre[u][h][0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rcond, co, 0, 0));
                            cpre[u][h][1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rcond, co + WN_H * 4u, 0, 0));
                        }
                }
            }
            lgkm_wait<0>(fa[1], fb[1]);
            mma(IC<1>{});                                      // slab 29
        }
        TLS();
        // ---- gate epilogue: (conv + b) -> dropout -> + conditioning -> tanh, sigmoid (Modules.py:861-870, 885-887) ----
        {
            int rb = rbw;
            asm volatile("" : "+v"(rb));                       // (opaque: the per-element invariants are not hoisted out of the layer loop - they spilled)
            const Rsrc rg = mk_rsrc(pick4(p.gates, l), keep ? (long)p.rows * (2 * WN_H * 2) : 0);
            const uint32_t rk0 = (uint32_t)(t0 + rb) * 0x9E3779B1u + seed0 + (uint32_t)l;      // drop_rowkey(seed, row) = fmix_head(row * M + seed)
            const uint32_t own0 = (uint32_t)(rb - halo);                                       // owned <=> (rb + c - halo) < lim (unsigned)
            unsigned char* const ac = AT + pi * (WN_WIN * 64) + rb * 64;
            const int* const ut = UT + rb + WN_PAD;
            uint32_t rkey[2][4];
            if constexpr (DROP) {
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        rkey[rt][i] = fmix_head(rk0 + (uint32_t)(16 * rt + i) * 0x9E3779B1u);
                    }
            }
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int jch = jch0 + 16 * h;
                const float b0 = BT[BT_IN + l * 384 + jch], b1 = BT[BT_IN + l * 384 + WN_H + jch];
                const uint32_t jkey = drop_colkey((uint32_t)jch);
                const uint32_t vg0 = (uint32_t)((t0 + rb) * (2 * WN_H * 2) + jch * 4);
                const int to = tile_off(h, 0);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) {
                    float c0[4], c1[4];
                    if constexpr (COND) {
                        if (two) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const bool lo = rb + WN_PAD + 16 * rt + i < cbnd;
                                c0[i] = lo ? cpre[0][h][0] : cpre[1][h][0]; c1[i] = lo ? cpre[0][h][1] : cpre[1][h][1];
                            }
                        } else {                               // per-row conditioning / short utterances: the 8 loads of 4 rows in flight together
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const uint32_t co = (uint32_t)(ut[16 * rt + i] * (int)p.ldcond + l * 2 * WN_H + jch) * 4u;
                                c0[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rcond, co, 0, 0));
                                c1[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rcond, co + WN_H * 4u, 0, 0));
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = 16 * rt + i;
                        float x0 = acc[rt][h][i] + b0, x1 = acc[rt][2 + h][i] + b1;
                        if constexpr (DROP) {
                            const uint32_t d = drop_draw(rkey[rt][i], jkey);
                            x0 *= drop_keep_lo(d, thr, ik); x1 *= drop_keep_hi(d, thr, ik);
                        }
                        if constexpr (COND) { x0 += c0[i]; x1 += c1[i]; }
                        const float tg = tanh_<false>(x0), sg = sigmoid_<false>(x1);
                        const bool ok = own0 + (uint32_t)c < (uint32_t)lim;
                        if constexpr (!(ABL & 8)) __builtin_amdgcn_raw_buffer_store_b32(pack_bf16x2(tg, sg), rg, ok ? vg0 + (uint32_t)(c * (2 * WN_H * 2)) : OOB, 0, 0);
                        *reinterpret_cast<unsigned short*>(ac + c * 64 + to) = bf16_bits(tg * sg);
                    }
                }
            }
        }
        TLS();
        if (!last) {
            // ---- Res_Skip_l: 1x1 on tanh * sigmoid, PAIR-packed columns: fragments 0, 1 = residual, 2, 3 = skip of channels [32 pi, 32 pi + 32) ----
            zero_acc();
            {
                Chunk16 fa[2][2], fb[2][4];                    // (pipelined like In_l)
                auto mma = [&](auto SET_) __attribute__((always_inline)) {
                    constexpr int st = decltype(SET_)::value;
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                        for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = mfma16_bf16<!(ABL & 2)>(fa[st][rt], fb[st][ct], acc[rt][ct]);
                };
#pragma unroll
                for (int kc = 0; kc < WN_KCH; ++kc) {
                    // behind the gate epilogue's XG stores; the copy-out's XC stores sit behind slab 0's wait; from step 3 on all are older
                    const unsigned char* slot = kc == 0 ? begin_step(IC<XG>{}) : (kc <= 2 ? begin_step(IC<keep ? XG + XC : XG>{}) : begin_step(IC<0>{}));
                    if (keep && kc == 0) copy_out(AT, WN_WIN, halo, pick4(p.acts, l));
                    const int st = kc & 1;
                    const uint32_t aa = lds_addr(AT) + (uint32_t)(kc * (WN_WIN * 64) + offA + bl), sa = lds_addr(slot) + (uint32_t)(offP + bl);
                    fa[st][0] = lds16_asm<0>(aa); fa[st][1] = lds16_asm<1024>(aa);
                    fb[st][0] = lds16_asm<0>(sa); fb[st][1] = lds16_asm<1024>(sa); fb[st][2] = lds16_asm<2048>(sa); fb[st][3] = lds16_asm<3072>(sa);
                    if (kc > 0) { lgkm_wait<6>(fa[st ^ 1], fb[st ^ 1]); if (st) mma(IC<0>{}); else mma(IC<1>{}); }
                    __builtin_amdgcn_sched_barrier(0);
                    end_step();
                }
                lgkm_wait<0>(fa[1], fb[1]);
                mma(IC<1>{});
            }
            TLS();
            // x_{l+1} = (x_l + res + b) * mask in place; skip += skip_l + b (Modules.py:871-879)
            int rb = rbw;
            asm volatile("" : "+v"(rb));
            unsigned char* const xc = XT + pi * (WN_XR * 64) + (rb + WN_PAD) * 64;
            const float* const mk = MK + rb + WN_PAD;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int jch = jch0 + 16 * h;
                const float br = BT[BT_RS + l * 384 + jch], bs = BT[BT_RS + l * 384 + WN_H + jch];
                const int to0 = tile_off(h, 0), to1 = tile_off(h, 1);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = 16 * rt + i;
                        unsigned short* xp = reinterpret_cast<unsigned short*>(xc + c * 64 + ((i + WN_PAD) >> 2 ? to1 : to0));
                        const float xin = __uint_as_float((uint32_t)*xp << 16);
                        *xp = bf16_bits((xin + acc[rt][h][i] + br) * mk[c]);
                        skp[rt][h][i] = skp[rt][h][i] + acc[rt][2 + h][i] + bs;
                    }
            }
        } else {
            // ---- last layer: Res_Skip has only skip outputs (192 columns: fragments ct = 0, 1 of this wave's 32 channels, two K chunks per slab) ----
            zero_acc();
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const unsigned char* slot = j == 0 ? begin_step(IC<XG>{}) : begin_step(IC<keep ? XG + XC : XG>{});
                if (keep && j == 0) copy_out(AT, WN_WIN, halo, pick4(p.acts, l));
                Chunk16 fa[2][2], fb[2][2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) fa[c][rt] = lds16(AT + (2 * j + c) * (WN_WIN * 64) + offA + rt * 1024 + bl);
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) fb[c][ct] = lds16(slot + c * 12288 + off1 + ct * 1024 + bl);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                        for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = mfma16_bf16<!(ABL & 2)>(fa[c][rt], fb[c][ct], acc[rt][ct]);
                __builtin_amdgcn_sched_barrier(0);
                end_step();
            }
            TLS();
            // output = (sum of skips + b) * mask (Modules.py:880-883): fp32 rows kept for the End conv's weight gradient, bf16 tile for the End conv
            int rb = rbw;
            asm volatile("" : "+v"(rb));
            const Rsrc rs = mk_rsrc(p.skip, (keep && p.skip) ? (long)p.rows * (WN_H * 4) : 0);
            const uint32_t own0 = (uint32_t)(rb - halo);
            unsigned char* const sc = XT + pi * (WN_WIN * 64) + rb * 64;
            const float* const mk = MK + rb + WN_PAD;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int jch = jch0 + 16 * h;
                const float b = BT[BT_RSL + jch];
                const uint32_t vs0 = (uint32_t)((t0 + rb) * (WN_H * 4) + jch * 4);
                const int to = tile_off(h, 0);
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = 16 * rt + i;
                        const float v = (skp[rt][h][i] + acc[rt][h][i] + b) * mk[c];
                        const bool ok = own0 + (uint32_t)c < (uint32_t)lim;
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, ok ? vs0 + (uint32_t)(c * (WN_H * 4)) : OOB, 0, 0);
                        *reinterpret_cast<unsigned short*>(sc + c * 64 + to) = bf16_bits(v);
                    }
            }
        }
    }

    TLS();
    // ================= End conv + affine coupling (Modules.py:793-806): PAIR-packed (m | logs), 6 waves x (32 rows x 64 packed columns) =================
    const int rfe = wave >= 3 ? 1 : 0, pe = wave - 3 * rfe;    // (waves 0..5 only)
    int laneE = lane;
    asm volatile("" : "+v"(laneE));                          // (opaque: nothing of this phase is computed early and kept live across the layers)
    const int l15e = laneE & 15, lqe = laneE >> 4;
    const int je0 = pe * 32 + l15e;                            // this lane's channels: je0 and je0 + 16
    const Rsrc rx = mk_rsrc(p.xsrc, (long)p.rows * p.ldx * 4), rz = mk_rsrc(p.xdst, (long)p.rows * p.ldxd * 4);
    int rbe = rfe * 32 + 4 * lqe;
    asm volatile("" : "+v"(rbe));
    const uint32_t owne = (uint32_t)(rbe - halo);
    float xb[2][2][4];                                         // [h][rt][i]
    {                                                          // (every wave issues the 16 loads - waves 6..11 out of range - so that the operation count below is uniform)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int je = je0 + 16 * h;
            const bool cok = wave < 6 && je < p.C2;
            const uint32_t vx0 = (uint32_t)((t0 + rbe) * (int)p.ldx + p.C2 + je) * 4u;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = 16 * rt + i;
                    const bool ok = cok && owne + (uint32_t)c < (uint32_t)lim;
                    xb[h][rt][i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, ok ? vx0 + (uint32_t)(c * (int)p.ldx * 4) : OOB, 0, 0));
                }
        }
    }
    zero_acc();
#pragma unroll
    for (int j = 0; j < 3; ++j) {                              // the last three slabs: the ring drains
        // behind these slabs' DMAs: the XG skip stores of the last epilogue and the 16 x_b loads
        if constexpr (SAFE) {
            if (j == 0)      asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else if (j == 1) asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            else             asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        } else {
            constexpr int XS = keep ? XC : 0;                  // the skip copy-out's stores, issued behind slab j = 0's wait
            if (j == 0)      asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(4 + XG + 16) : "memory");
            else if (j == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(2 + XG + 16 + XS) : "memory");
            else             asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(XG + 16 + XS) : "memory");
        }
        const unsigned char* slot = wn_smem + OFF_RING + (snext & (WN_NS - 1)) * WN_SLAB;
        ++snext;
        // the bf16 skip sum (the End conv's operand tile) also goes out: X of the End conv's weight gradient at half the bytes (a null pointer
        // gives an empty descriptor: the two stores are issued and dropped, the counts above stay static)
        if (keep && j == 0) copy_out(XT, WN_WIN, halo, p.skip_bf);
        if (wave < 6) {
            const int ble = swz16(l15e, lqe);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const unsigned char* At = XT + (2 * j + c) * (WN_WIN * 64);
                Chunk16 fa[2], fb[4];
#pragma unroll
                for (int rt = 0; rt < 2; ++rt) fa[rt] = lds16(At + rfe * 2048 + rt * 1024 + ble);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) fb[ct] = lds16(slot + c * 12288 + pe * 4096 + ct * 1024 + ble);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int rt = 0; rt < 2; ++rt) acc[rt][ct] = mfma16_bf16<!(ABL & 2)>(fa[rt], fb[ct], acc[rt][ct]);
            }
        }
    }
    TLS();
    if (wave < 6) {
        const Rsrc ro = mk_rsrc(p.outs, keep ? (long)p.rows * p.ldo * 4 : 0);
        const bool rev = p.reverse != 0;
        const float* const mk = MK + rbe + WN_PAD;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int je = je0 + 16 * h;
            const bool cok = je < p.C2;
            const float bm = cok ? BT[BT_END + je] : 0.f, bls = cok ? BT[BT_END + p.C2 + je] : 0.f;
            const uint32_t vz0 = (uint32_t)((t0 + rbe) * (int)p.ldxd + p.C2 + je) * 4u, vo0 = (uint32_t)((t0 + rbe) * (int)p.ldo + pe * 64 + 16 * h + l15e) * 4u;
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = 16 * rt + i;
                    const bool ok = cok && owne + (uint32_t)c < (uint32_t)lim;
                    const float m = acc[rt][h][i] + bm, lg = acc[rt][2 + h][i] + bls;
                    const float z = rev ? (xb[h][rt][i] - m) * exp_<false>(-lg) * mk[c] : (m + exp_<false>(lg) * xb[h][rt][i]) * mk[c];
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(z), rz, ok ? vz0 + (uint32_t)(c * (int)p.ldxd * 4) : OOB, 0, 0);
                    const uint32_t vo = ok ? vo0 + (uint32_t)(c * (int)p.ldo * 4) : OOB;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m), ro, vo, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(lg), ro, vo + 128u, 0, 0);
                    xb[h][rt][i] = z;                               // (kept for the next flow's ActNorm + 1x1 below)
                }
        }
    }
    // ---- the NEXT flow's ActNorm + invertible 1x1 conv on the rows just produced (flow_ops.hip actnorm_inv_kernel's arithmetic and access pattern):
    // z_b of the window goes through the ring slot no slab occupies any more, then ALL twelve waves take (row, channel group) items: group g mixes
    // (x_a[2g], x_a[2g+1], z_b[2g], z_b[2g+1]) - float2 loads and stores, contiguous over g.  (Done from the accumulator layout by the six End waves alone -
    // 4-byte scattered stores, every pair computed twice - the epilogue cost as much as the launch it replaces.) ----
    if (p.nx_xmid && p.reverse == 0) {
        float* const Z = reinterpret_cast<float*>(wn_smem + OFF_RING + (snext & (WN_NS - 1)) * WN_SLAB);      // [64 window rows][ZLD]
        constexpr int ZLD = 96;
        if (wave < 6) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int je = je0 + 16 * h;
#pragma unroll
                for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                    for (int i = 0; i < 4; ++i) Z[(rbe + 16 * rt + i) * ZLD + je] = xb[h][rt][i];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const int Cn = 2 * p.C2, G = p.C2 >> 1;
        const Rsrc rnm = mk_rsrc(p.nx_xmid, (long)p.rows * Cn * 4), rno = mk_rsrc(p.nx_xout, (long)p.rows * Cn * 4);
        const Rsrc rnb = mk_rsrc(p.nx_xa_bf, p.nx_xa_bf ? (long)p.rows * p.C2 * 2 : 0);
        float w[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) w[q] = p.nx_winfo[q];
        const int nitems = lim * G;
        for (int it = tid; it < nitems; it += WN_NT) {
            const int r = it / G, g = it - r * G;                // owned row r = window row halo + r = global row v0 + r
            const int grow = v0 + r;
            const float m = MK[halo + r + WN_PAD];
            const uint32_t vsrc = (uint32_t)(grow * (int)p.ldx + 2 * g) * 4u;
            float x[4], e[4], bsn[4], o[4];
            x[0] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, vsrc, 0, 0));
            x[1] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rx, vsrc, 4, 0));
            x[2] = Z[(halo + r) * ZLD + 2 * g];
            x[3] = Z[(halo + r) * ZLD + 2 * g + 1];
            const int ch[4] = {2 * g, 2 * g + 1, p.C2 + 2 * g, p.C2 + 2 * g + 1};
#pragma unroll
            for (int k = 0; k < 4; ++k) { e[k] = expf(p.nx_logs[ch[k]]); bsn[k] = p.nx_bias[ch[k]]; }
            actnorm_mix4(x, e, bsn, w, m, o);
            const uint32_t vn = (uint32_t)(grow * Cn + 2 * g) * 4u;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[0]), rnm, vn, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[1]), rnm, vn, 4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[2]), rnm, vn + (uint32_t)p.C2 * 4u, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[3]), rnm, vn + (uint32_t)p.C2 * 4u, 4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[0]), rno, vn, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[1]), rno, vn, 4, 0);
            __builtin_amdgcn_raw_buffer_store_b32(pack_bf16x2(o[0], o[1]), rnb, (uint32_t)(grow * p.C2 + 2 * g) * 2u, 0, 0);
        }
    }
    TLS();
}

template <bool DROP, bool COND, bool KEEP, bool SAFE = false, int ABL = 0>
int launch_wn_fwd(const wn_fwd_args& k, dim3 grid, hipStream_t s)
{
#ifdef GLOWTTS_TOOLS
    if constexpr (ABL == 0 && !COND && KEEP && !SAFE) {
        switch (GLOWTTS_TUNABLE("GLOWTTS_WN_ABL", 0)) {
            case 1: return launch_wn_fwd<DROP, COND, KEEP, SAFE, 1>(k, grid, s);
            case 2: return launch_wn_fwd<DROP, COND, KEEP, SAFE, 2>(k, grid, s);
            case 3: return launch_wn_fwd<DROP, COND, KEEP, SAFE, 3>(k, grid, s);
            case 4: return launch_wn_fwd<DROP, COND, KEEP, SAFE, 4>(k, grid, s);
            case 16: return launch_wn_fwd<DROP, COND, KEEP, SAFE, 16>(k, grid, s);
            case 8: return launch_wn_fwd<DROP, COND, KEEP, SAFE, 8>(k, grid, s);
            case 32: return launch_wn_fwd<DROP, COND, KEEP, SAFE, 32>(k, grid, s);
            case 40: return launch_wn_fwd<DROP, COND, KEEP, SAFE, 40>(k, grid, s);
            default: break;
        }
    }
#endif
    static bool attr_done = false;
    if (!attr_done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&wn_fwd_kernel<DROP, COND, KEEP, SAFE, ABL>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return GLOWTTS_E_LAUNCH;
        attr_done = true;
    }
    GLOWTTS_NOTE_STATIC("wn_fwd<%s%s>", DROP ? "drop" : "nodrop", COND ? ",cond" : "");
    hipLaunchKernelGGL((wn_fwd_kernel<DROP, COND, KEEP, SAFE, ABL>), grid, dim3(WN_NT), WN_LDS, s, k);
    RET_LAUNCH();
}

template <bool DROP, bool COND>
int launch_wn_fwd_keep(const wn_fwd_args& k, dim3 grid, hipStream_t s)
{
    if (k.keep) {
        if constexpr (!COND) { if (k.safe_waits) return launch_wn_fwd<DROP, COND, true, true>(k, grid, s); }      // (test hook: conservative waits, unconditioned training shape only)
        return launch_wn_fwd<DROP, COND, true>(k, grid, s);
    }
    return launch_wn_fwd<DROP, COND, false>(k, grid, s);
}

}  // namespace

int glowtts_wavenet_pack_bwd_images(const float* w_start, const float* w_in, const float* w_rs, const float* w_rs_last, const float* w_end,
                                    int F, int L, int C2, void* img_bwd, void* stream);      // wavenet_fused_bwd.hip
static int g_wn_safe_waits = 0;
extern "C" void glowtts_wavenet_debug_safe_waits(int on) { g_wn_safe_waits = on ? 1 : 0; }
int glowtts_wavenet_safe_waits_flag() { return g_wn_safe_waits; }

extern "C" int glowtts_wavenet_image_bytes(int L, int transposed, int64_t* bytes_out)
{
    if (L < 1 || L > WN_MAXL || !bytes_out) return GLOWTTS_E_ARG;
    (void)transposed;
    *bytes_out = (int64_t)(36 * L + 2) * WN_SLAB;
    return GLOWTTS_OK;
}

extern "C" int glowtts_wavenet_pack_images(const float* w_start, const float* w_in, const float* w_rs, const float* w_rs_last, const float* w_end,
                                           int F, int L, int C2, void* img_fwd, void* img_bwd, void* stream)
{
    if (!w_start || !w_in || !w_rs_last || !w_end || (L > 1 && !w_rs) || F < 1 || L < 1 || L > WN_MAXL || C2 <= 64 || C2 > 96 || (C2 & 3)) return GLOWTTS_E_ARG;
    const int H = WN_H;
    const int64_t stride = (int64_t)(36 * L + 2) * WN_SLAB;
    if (img_fwd) {
        unsigned char* img = static_cast<unsigned char*>(img_fwd);
        // [Start: 2 slabs][layer l: In_l 30 slabs, Res_Skip_l 6 slabs (last layer: 3)][End: 3 slabs]
        int rc = glowtts_pack_weight_strided(w_start, F, 1, H, C2, 1, 0, GLOWTTS_PERM_NONE, 0, GLOWTTS_BF16, img, stride, 0, 0, stream);
        if (rc == GLOWTTS_OK) rc = glowtts_pack_weight_strided(w_in, F * L, L, 2 * H, H, WN_TAPS, 0, GLOWTTS_PERM_PAIR, H, GLOWTTS_BF16, img + 2 * WN_SLAB, stride, 36 * (int64_t)WN_SLAB, 0, stream);
        if (rc == GLOWTTS_OK && L > 1) rc = glowtts_pack_weight_strided(w_rs, F * (L - 1), L - 1, 2 * H, H, 1, 0, GLOWTTS_PERM_PAIR, H, GLOWTTS_BF16, img + 32 * WN_SLAB, stride, 36 * (int64_t)WN_SLAB, 0, stream);
        if (rc == GLOWTTS_OK) rc = glowtts_pack_weight_strided(w_rs_last, F, 1, H, H, 1, 0, GLOWTTS_PERM_NONE, 0, GLOWTTS_BF16, img + (int64_t)(36 * (L - 1) + 32) * WN_SLAB, stride, 0, 0, stream);
        if (rc == GLOWTTS_OK) rc = glowtts_pack_weight_strided(w_end, F, 1, 2 * C2, H, 1, 0, GLOWTTS_PERM_PAIR, C2, GLOWTTS_BF16, img + (int64_t)(36 * (L - 1) + 35) * WN_SLAB, stride, 0, 0, stream);
        if (rc != GLOWTTS_OK) return rc;
    }
    if (img_bwd) return glowtts_wavenet_pack_bwd_images(w_start, w_in, w_rs, w_rs_last, w_end, F, L, C2, img_bwd, stream);
    return GLOWTTS_OK;
}

extern "C" int glowtts_wavenet_fwd(const glowtts_flow_dims* d, const glowtts_flow_params* p, const glowtts_flow_acts* a,
                                   const float* xsrc, float* xdst, int reverse, int keep, void* stream)
{
    if (!d || !p || !a || !xsrc || !xdst || !p->wn_img || !a->rowmask) return GLOWTTS_E_ARG;
    const int C2 = d->C / 2;
    if (d->precision != GLOWTTS_BF16 || !d->act_bf16 || d->H != WN_H || d->ksize != WN_TAPS || d->L < 1 || d->L > WN_MAXL ||
        (d->C & 7) || C2 <= 64 || C2 > 96 || p->end.npad != 192 || p->start.kchunks != 3) return GLOWTTS_E_ARG;
    const int Tp = d->T + 2 * GLOWTTS_ROW_PAD;
    const int64_t R = (int64_t)d->B * Tp;
    if (R * 2 * WN_H * 2 >= ((int64_t)1 << 31) || R * d->C * 4 >= ((int64_t)1 << 31)) return GLOWTTS_E_ARG;
    if (p->cond && ((p->cond_rows ? R : (int64_t)d->B) * p->ldcond * 4 >= ((int64_t)1 << 31))) return GLOWTTS_E_ARG;   // 32-bit buffer offsets (per-row / per-utterance table)
    wn_fwd_args k;
    memset(&k, 0, sizeof(k));
    k.rows = (int)R; k.rows_per_utt = Tp; k.L = d->L; k.C2 = C2; k.reverse = reverse; k.keep = keep;
    k.xsrc = xsrc; k.ldx = d->C; k.xdst = xdst; k.ldxd = d->C; k.rowmask = a->rowmask;
    if (a->next_xmid && !reverse) {                           // the next flow's ActNorm + 1x1 in this launch's coupling epilogue (glowtts_flow_acts.next_*)
        if (!a->next_an_logs || !a->next_an_bias || !a->next_winfo || !a->next_xout) return GLOWTTS_E_ARG;
        k.nx_logs = a->next_an_logs; k.nx_bias = a->next_an_bias; k.nx_winfo = a->next_winfo;
        k.nx_xmid = a->next_xmid; k.nx_xout = a->next_xout; k.nx_xa_bf = static_cast<uint32_t*>(a->next_xa_bf);
    }
    k.wimg = static_cast<const unsigned char*>(p->wn_img);
    k.b_start = p->b_start; k.b_end = p->b_end;
    for (int l = 0; l < d->L; ++l) { k.b_in[l] = p->b_in[l]; k.b_rs[l] = p->b_rs[l]; }
    k.cond = p->cond; k.ldcond = p->ldcond; k.cond_rows = p->cond_rows;
    k.drop_p = d->drop_p; k.seed = d->seed; k.seed_ptr = d->seed_ptr;
    k.safe_waits = g_wn_safe_waits;
#ifdef GLOWTTS_TOOLS
    if (GLOWTTS_TUNABLE("GLOWTTS_WN_ABL", 0) & 16) k.tl = reinterpret_cast<long long*>(a->skip_bf);      // tools/bench_wn.py passes the stamp buffer here
    k.stagger = GLOWTTS_TUNABLE("GLOWTTS_WN_STAGGER", 0);
#endif
    if (keep) {
        // (a->skip == NULL, round 5: the fp32 skip rows are not kept - the caller's backward reads the bf16 copy skip_bf only; the epilogue's 16 stores then
        // fall outside a zero-sized buffer range and are dropped by the bounds check, 9.9 MB per launch at B = 32)
        if ((!a->skip && !a->skip_bf) || !a->outs) return GLOWTTS_E_ARG;
        for (int l = 0; l < d->L; ++l) {
            if (!a->hs[l] || !a->gates[l] || !a->acts[l]) return GLOWTTS_E_ARG;
            k.hs[l] = a->hs[l]; k.gates[l] = a->gates[l]; k.acts[l] = a->acts[l];
        }
        k.skip = a->skip; k.outs = a->outs; k.ldo = p->end.npad; k.skip_bf = a->skip_bf;
    }
    const int nvalid = WN_WIN - 2 * WN_PAD * (d->L - 1);
    const dim3 grid((unsigned)((R + nvalid - 1) / nvalid));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool drop = d->drop_p > 0.f, cnd = p->cond != nullptr;
    if (drop && cnd) return launch_wn_fwd_keep<true, true>(k, grid, s);
    if (drop) return launch_wn_fwd_keep<true, false>(k, grid, s);
    if (cnd) return launch_wn_fwd_keep<false, true>(k, grid, s);
    return launch_wn_fwd_keep<false, false>(k, grid, s);
}
