// xq_conv_block_c8.h -- part of xq_conv.hip's translation unit; do not compile it into a second one: the unit's device code is
// compared kernel by kernel when text moves between these headers (EXPERIMENTS.md, "the convolution unit's text in headers"), and
// the search unit's kernels changed by 0.4-1.7 % when part of that unit was compiled alone.
//
// Kernel 2c8: k_resblock_c8, the residual block on the c8 / c6 arithmetic (rb8:: LDS layout and Shadow, the RB_STAMP timing hooks of
// the CZ_RB_STAMPS variant build), optionally with the fused input layer (FIRST) or the head convolutions (HEADS).
#pragma once
#include "xq_c8_kloop.h"
#include "xq_conv_kloop.h"

namespace {

#ifdef CZ_RB_STAMPS
// timing build (tools/rb_stamps.py; never the default library): shader-cycle stamps of one matrix wave's and one copy
// wave's sections of one steady-state board of k_resblock_c8
__device__ long long g_rb_stamps[32];
#define RB_STAMP(i) do { if (stamp_on) g_rb_stamps[i] = clock64(); } while (0)
#else
#define RB_STAMP(i) do { } while (0)
#endif

// ---- kernel 2c8: the residual block on the c8 arithmetic (round 4) -------------------------------------------------------
// k_resblock's roles and LDS images (X | Y | fp32 staging; 4 matrix waves + 4 copy waves, one workgroup per CU), with the
// critical path of a board cut down to what in-kernel cycle stamps showed it to be (tools/rb_stamps.py on round 3's
// schedule: 44.2 k shader cycles per board = two K loops 20.0 + 16.2 k, epilogue 1 3.8 k, epilogue 2 2.8 k, 1.2 k waiting for
// the copy waves to hand X over):
//   * accumulators START at bias (K loop 1) and at bias + skip (K loop 2; read from X by the lane that owns the element,
//     unit by unit as epilogue 1 frees the registers): no additions left in the epilogues, and X is dead once K loop 2 starts;
//   * epilogue 2 is only  relu -> fp32 staging  and is DEFERRED into the fp8 slots of the next board's first K loop
//     (12 ds_write_b128 per wave, one every ninth slot; c8k::kloop's shadow hook) -- the conversion to the c8 triple stays
//     with the copy waves, whose instructions do not compete with the matrix waves' issue slots the way shadow VALU work
//     does (the fully in-place pipelined form, 45 VALU per unit in the shadow, measured 7 % SLOWER than the plain one);
//   * the copy waves write the next board into X during K loop 2 (X is free from barrier B on) and store the previous
//     board from the staging image there too; under K loop 1 they only issue the next board's loads.  Two barriers per
//     board instead of three, none of them waited at by the matrix waves.
//   matrix waves, board k:  A | K1(k) + shadow: staging <- relu(acc2(k-1)) | epi1 -> Y, acc <- b2 + skip | B | K2(k) | ...
//   copy waves:             A | loads of board k+1 -> registers            |                            | B | store board
//                               k-1 from staging (c8 split, or fp32, or the head convolutions); X <- board k+1
// FIRST: the block is the first of the tower; its copy waves compute the 5 x 5 input layer of board k+1 as an fp32 gather
// over the occupied squares (see k_resblock_pipe<FIRST>, csrc/xq_conv_pipe.h: the same algorithm, here producing the c8 triple) instead
// of loading it.  HEADS: the last block; the copy waves apply the two 1 x 1 head convolutions to the staged activation.
// Arithmetic and its order are k_conv3x3_c8's: bit-identical to two cz_conv3x3_c8 launches.
constexpr int CZ_FIRST_PRIO = 3;   // issue priority of the copy waves while they compute the fused input layer (the matrix waves
                                   // run their K loops at 3; at 0 the gather starves: first block 3.53 -> 3.48 ms)
namespace rb8 {
constexpr int C = 128, ZROW = 96, PART = (ZROW + 16) * RB, REGION = 2 * PART;
constexpr int SROW = 512, S_BYTES = 90 * SROW;
constexpr int Y_OFF = REGION, S_OFF = 2 * REGION, BIAS_OFF = S_OFF + S_BYTES, MASK_OFF = BIAS_OFF + 2 * C * 4;
constexpr int LDS_BYTES = MASK_OFF + 4 * 96 * 4;
constexpr int DUMP_OFF = Y_OFF + 90 * RB;      // rows 90 .. 95 of Y are never read: the shadow's padding lanes write here
static_assert(LDS_BYTES <= 160 * 1024, "X + Y + staging + bias + mask boards must fit the CU's LDS");
// staging offset of channels ch .. ch + 3 of pixel q (fp32, 32 chunks of 16 bytes per row, swizzled by the row)
__device__ __forceinline__ int stage_off(int q, int ch) { return q * SROW + ((((ch >> 2) & ~7) | (((ch >> 2) ^ q) & 7)) << 4); }

struct Shadow {                         // relu(acc2 of the previous board) -> staging, one (tile, channel group) unit per 9 fp8 slots
    unsigned char* lds;
    f32x16* prev;                       // the body always reads prev[0]; rotated at the end of an iteration
    int wave, kb, ln;
    __device__ __forceinline__ void unit(const f32x16& a, int q, int g)
    {
        const int ch = wave * 32 + g * 8 + kb * 4;
        const int addr = q < 90 ? S_OFF + stage_off(q, ch) : DUMP_OFF + (kb * 6 + (ln - 26)) * 16;
        float4 v;
        v.x = a[g * 4 + 0] > 0.0f ? a[g * 4 + 0] : 0.0f;
        v.y = a[g * 4 + 1] > 0.0f ? a[g * 4 + 1] : 0.0f;
        v.z = a[g * 4 + 2] > 0.0f ? a[g * 4 + 2] : 0.0f;
        v.w = a[g * 4 + 3] > 0.0f ? a[g * 4 + 3] : 0.0f;
        *reinterpret_cast<float4*>(lds + addr) = v;
    }
    __device__ __forceinline__ void fp8(int j, int slot)
    {
        if (slot % 9 == 4) unit(prev[0], j * 32 + ln, slot / 9);
        if (slot == 35) {
            prev[0] = prev[1];
            prev[1] = prev[2];
        }
    }
};
}  // namespace rb8

template <bool FIRST, bool HEADS, bool C6 = false>
__global__ __launch_bounds__(512, 2) void k_resblock_c8(
    const _Float16* __restrict__ xh, const unsigned char* __restrict__ xc, const void* __restrict__ w1p,
    const float* __restrict__ b1, const void* __restrict__ w2p, const float* __restrict__ b2, _Float16* __restrict__ yh,
    unsigned char* __restrict__ yc, float* __restrict__ yf, int n_boards, HeadArgs hd, const int32_t* __restrict__ n_dev,
    FirstArgs fa)
{
    using namespace rb8;
    static_assert(!(FIRST && HEADS), "a one-block tower runs cz_input_conv + the HEADS block");
    typedef Geom<C, 1, 2> G;
    static_assert(G::ZROW == ZROW && G::PART_BYTES == PART && G::REGION == REGION, "LDS image geometry");
    constexpr int NT = 3, CTHR = 256, CHUNKS = 90 * 16, LITER = (CHUNKS + CTHR - 1) / CTHR;
    constexpr int PIECES = 90 * (C / 8), EITER = (PIECES + CTHR - 1) / CTHR;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    n_boards = nn_live_boards(n_boards, n_dev);
    unsigned char* X = lds;
    unsigned char* Y = lds + Y_OFF;
    unsigned char* S = lds + S_OFF;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = gridDim.x;
    int t = blockIdx.x;
    if (t >= n_boards) return;

    if (wave >= 4) {                                    // ---- copy waves ----
        const int ctid = tid - 256;
        uint4 v[2][LITER];
        float hw[HEADS ? 6 : 1][8];                     // this thread's slice of the head filters
        if (HEADS) {
#pragma unroll
            for (int o = 0; o < 6; ++o)
#pragma unroll
                for (int k = 0; k < 8; ++k) hw[o][k] = hd.w[o * C + (ctid % (C / 8)) * 8 + k];
        }
        // board `to` from the staging image (fp32, already ReLU'd) to HBM
        auto store_tile = [&](int to, int ct2) __attribute__((always_inline)) {
            const size_t ebase = (size_t)to * 90 * C;
#pragma unroll
            for (int it = 0; it < EITER; ++it) {
                const int i = it * CTHR + ct2;
                if (!((it + 1) * CTHR <= PIECES || i < PIECES)) continue;
                const int qq = i / (C / 8), c8 = i % (C / 8);
                const float4 f0 = *reinterpret_cast<const float4*>(S + stage_off(qq, c8 * 8));
                const float4 f1 = *reinterpret_cast<const float4*>(S + stage_off(qq, c8 * 8 + 4));
                const float r[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                if (HEADS) {
                    // 16 consecutive lanes hold the 128 channels of one pixel: partial dot products, then a 16-lane
                    // butterfly; lane o of the group writes head output o
                    float hs[6];
#pragma unroll
                    for (int o = 0; o < 6; ++o) {
                        float a = 0.0f;
#pragma unroll
                        for (int k = 0; k < 8; ++k) a += r[k] * hw[o][k];
                        a = row16_sum(a);
                        hs[o] = a;
                    }
#pragma unroll
                    for (int o = 0; o < 6; ++o)
                        if (c8 == o) {
                            float hv = hs[o] + hd.b[o];
                            hv = hv > 0.0f ? hv : 0.0f;
                            if (o < hd.n_pol) hd.pol[(size_t)to * (hd.n_pol * 90) + o * 90 + qq] = hv;
                            else hd.val[(size_t)to * ((6 - hd.n_pol) * 90) + (o - hd.n_pol) * 90 + qq] = hv;
                        }
                } else if (yf) {
                    float4* o = reinterpret_cast<float4*>(yf + ebase) + 2 * i;
                    o[0] = f0;
                    o[1] = f1;
                } else {
                    const cf8::Split4 s0 = cf8::split4(r), s1 = cf8::split4(r + 4);
                    struct alignas(16) H8 { Quad<_Float16> a, b; };
                    reinterpret_cast<uint4*>(yh + ebase)[i] = __builtin_bit_cast(uint4, H8{s0.hi, s1.hi});
                    unsigned char* row = yc + ebase * 2 + (size_t)qq * 2 * C + c8 * 8;
                    *reinterpret_cast<uint2*>(row) = make_uint2(s0.l8, s1.l8);
                    *reinterpret_cast<uint2*>(row + C) = make_uint2(s0.h8, s1.h8);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // the same for a c6 output image.  Pass A: the f16 halves in store_tile's mapping (a thread = 8 channels of a pixel:
        // 16 bytes, consecutive over the lanes -- whole cache lines per instruction).  Pass B: one thread takes the 32 channels
        // of a (pixel, block) -- a whole piece of each kind (24 bytes, 4 neighbouring lanes fill 96 of a line's 128).
        // (The K loops' filter stream keeps the CU's vector-memory path ~80 % busy -- 576 KB per board and convolution at
        //  64 B/clk --, so every extra memory instruction of the copy waves shows: an earlier form that wrote the f16 halves
        //  from pass B's mapping, 16 bytes at a 64-byte lane stride, cost 0.1 ms per launch more; streaming (nt) stores 0.13.)
        const int k_out = C6 ? __builtin_amdgcn_readfirstlane(pack_ints(w2p)[3]) : 0;
        auto store_tile_c6 = [&](int to, int ct2) __attribute__((always_inline)) {
            const size_t ebase = (size_t)to * 90 * C;
            const float s_hi = __builtin_ldexpf(1.0f, k_out), s_lo = __builtin_ldexpf(1.0f, k_out - cf8::X_LO_SHIFT);
            struct alignas(16) H8 { Quad<_Float16> a, b; };
#pragma unroll
            for (int it = 0; it < EITER; ++it) {               // ---- pass A
                const int i = it * CTHR + ct2;
                if (!((it + 1) * CTHR <= PIECES || i < PIECES)) continue;
                const int qq = i / (C / 8), c8 = i % (C / 8);
                const float4 f0 = *reinterpret_cast<const float4*>(S + stage_off(qq, c8 * 8));
                const float4 f1 = *reinterpret_cast<const float4*>(S + stage_off(qq, c8 * 8 + 4));
                H8 h;
                h.a.e[0] = (_Float16)f0.x; h.a.e[1] = (_Float16)f0.y; h.a.e[2] = (_Float16)f0.z; h.a.e[3] = (_Float16)f0.w;
                h.b.e[0] = (_Float16)f1.x; h.b.e[1] = (_Float16)f1.y; h.b.e[2] = (_Float16)f1.z; h.b.e[3] = (_Float16)f1.w;
                reinterpret_cast<uint4*>(yh + ebase)[i] = __builtin_bit_cast(uint4, h);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int it = 0; it < 2; ++it) {                   // ---- pass B
                const int i = it * CTHR + ct2;
                if (i >= 90 * 4) continue;
                const int qq = i >> 2, blk = i & 3;
                f32x16 av, bv, al, bl;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 f0 = *reinterpret_cast<const float4*>(S + stage_off(qq, blk * 32 + 8 * k));
                    const float4 f1 = *reinterpret_cast<const float4*>(S + stage_off(qq, blk * 32 + 8 * k + 4));
                    const float r[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        av[4 * k + j] = r[j];
                        bv[4 * k + j] = r[4 + j];
                        al[4 * k + j] = r[j] - (float)(_Float16)r[j];
                        bl[4 * k + j] = r[4 + j] - (float)(_Float16)r[4 + j];
                    }
                }
                const u32x6 pl = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(al, bl, s_lo);
                const u32x6 pv = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(av, bv, s_hi);
                unsigned char* row = yc + ebase * 2 + (size_t)qq * 2 * C;
                *reinterpret_cast<uint4*>(row + 16 * c6_chunk(0, blk)) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
                *reinterpret_cast<uint2*>(row + 16 * c6_chunk(0, blk) + 16) = make_uint2(pl[4], pl[5]);
                *reinterpret_cast<uint4*>(row + 16 * c6_chunk(1, blk)) = make_uint4(pv[0], pv[1], pv[2], pv[3]);
                *reinterpret_cast<uint2*>(row + 16 * c6_chunk(1, blk) + 16) = make_uint2(pv[4], pv[5]);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        // (two call sites each; a wrapper lambda around them was NOT inlined by the compiler: a call inside the kernel, 2.5x
        //  the scratch and 17 % of the launch time)
        // (k_out == CZ_C6_OUT_C8: the last c6 block of a hybrid c6>N tower hands a c8 image to the c8 blocks behind it)
#define CZ_STORE_BOARD(to, ct2) do { if (C6 && !HEADS && !yf && k_out != CZ_C6_OUT_C8) store_tile_c6(to, ct2); else store_tile(to, ct2); } while (0)
        // registers -> X image.  Loaded boards: 16-byte chunks of both parts; FIRST: the thread's 8 channels of a pixel are
        // one 16-byte chunk of the f16 row and two 8-byte pieces of the c8 row [lo8 x 128 | e4m3(x) x 128]
        auto write_x = [&](int ct2) {
#pragma unroll
            for (int it = 0; it < LITER; ++it) {
                const int i = it * CTHR + ct2;
                if (!((it + 1) * CTHR <= CHUNKS || i < CHUNKS)) continue;
                const int row = i >> 4, ch = i & 15;
                *reinterpret_cast<uint4*>(X + row * RB + ((ch ^ (row & 15)) << 4)) = v[0][it];
                if (FIRST) {
                    unsigned char* r = X + PART + row * RB + (ch & 1) * 8;
                    *reinterpret_cast<uint2*>(r + (((ch >> 1) ^ (row & 15)) << 4)) = make_uint2(v[1][it].x, v[1][it].y);
                    *reinterpret_cast<uint2*>(r + (((8 + (ch >> 1)) ^ (row & 15)) << 4)) = make_uint2(v[1][it].z, v[1][it].w);
                } else {
                    *reinterpret_cast<uint4*>(X + PART + row * RB + ((ch ^ (row & 15)) << 4)) = v[1][it];
                }
            }
        };
        // ---- FIRST: the input layer of a board into v[][], in two halves (k_resblock_pipe<FIRST>, csrc/xq_conv_pipe.h, documents the
        // algorithm).  planes_prefetch, first_begin and first_rounds are that kernel's, statement for statement: a change to one goes
        // into the other.  (One shared definition -- a struct owning the state, or functions over it -- was tried in nine forms: each
        // changed the scratch size of FIRST instantiations, EXPERIMENTS.md.)
        float acc[FIRST ? LITER : 1][8];
        uint32_t occ[FIRST ? LITER : 1], cur_m[FIRST ? LITER : 1];
        int cur_tap[FIRST ? LITER : 1];
        uint32_t* mk = reinterpret_cast<uint32_t*>(lds + MASK_OFF) + (wave - 4) * 96;     // this wave's own mask board
        const int c8 = ctid & 15, prow = ctid >> 4;            // chunk = channels 8 c8 .. 8 c8 + 7 of pixels prow + 16 it
        constexpr int PW = 12;                                 // plane words per lane: 32 planes x 90 bytes / 4 / 64 lanes
        uint32_t pw[FIRST ? PW : 1];
        auto planes_prefetch = [&](int board) {
            const int per_board = fa.in_planes * 90;
            const size_t slot = (size_t)(fa.rows ? fa.rows[board] : board);
            if (fa.masks) {                                    // the board's occupancy board, as the search kernel wrote it
                pw[0] = fa.masks[slot * 96 + lane];
                if constexpr (FIRST) pw[1] = lane < 32 ? fa.masks[slot * 96 + 64 + lane] : 0u;      // (pw is one word without FIRST)
                return;
            }
            const uint32_t* src = reinterpret_cast<const uint32_t*>(fa.planes + slot * per_board);
#pragma unroll
            for (int j = 0; j < PW; ++j) {
                const int w = lane + 64 * j;
                pw[j] = w < per_board / 4 ? src[w] : 0u;
            }
        };
        auto first_begin = [&]() {
            if (fa.masks) {                                    // (round 5) the mask board arrives ready-made
                mk[lane] = pw[0];
                if constexpr (FIRST) {
                    if (lane < 32) mk[64 + lane] = pw[1];
                }
            } else {
                mk[lane] = 0u;
                if (lane < 32) mk[64 + lane] = 0u;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int j = 0; j < PW; ++j) {
                    const int w = lane + 64 * j;
                    const uint32_t word = pw[j];
                    if (word == 0u) continue;
                    int c = (w * 4) / 90, pix = w * 4 - c * 90;
#pragma unroll
                    for (int k4 = 0; k4 < 4; ++k4) {
                        if ((word >> (8 * k4)) & 0xFFu) atomicOr(&mk[pix], 1u << c);
                        if (++pix == 90) { pix = 0; ++c; }
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_wave_barrier();
            const uint64_t occ_lo = __ballot(mk[lane] != 0u);
            const uint64_t occ_hi = __ballot(lane < 26 && mk[64 + (lane & 31)] != 0u);
            const float4 b0 = *reinterpret_cast<const float4*>(fa.in_bias + c8 * 8);
            const float4 b1v = *reinterpret_cast<const float4*>(fa.in_bias + c8 * 8 + 4);
#pragma unroll
            for (int it = 0; it < LITER; ++it) {
                acc[it][0] = b0.x; acc[it][1] = b0.y; acc[it][2] = b0.z; acc[it][3] = b0.w;
                acc[it][4] = b1v.x; acc[it][5] = b1v.y; acc[it][6] = b1v.z; acc[it][7] = b1v.w;
                const int p = prow + 16 * it;
                const int py = p / 9, px = p - py * 9;
                uint32_t o = 0u;
                if (p < 90) {
#pragma unroll
                    for (int ky = 0; ky < 5; ++ky) {
                        const int r = py + ky - 2;
                        if ((unsigned)r < 10u) {
                            const int sh = r * 9;
                            const uint32_t rowbits = (uint32_t)((sh < 64 ? (occ_lo >> sh) | (sh > 55 ? occ_hi << (64 - sh) : 0ull)
                                                                         : occ_hi >> (sh - 64)) & 0x1FFull);
                            o |= (((rowbits << 2) >> px) & 31u) << (5 * ky);
                        }
                    }
                }
                occ[it] = o;
                cur_m[it] = 0u;
                cur_tap[it] = 0;
            }
        };
        // one table row per chunk and ROUND, a round being one L2 round trip (two rows per round: rejected, EXPERIMENTS.md)
        auto first_rounds = [&](int max_rounds) {
#pragma unroll 1
            for (int round = 0; round < max_rounds; ++round) {
                uint32_t any = 0u;
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    if (cur_m[it] == 0u && occ[it] != 0u) {
                        const int tap = __builtin_ctz(occ[it]);
                        occ[it] &= occ[it] - 1u;
                        const int p = prow + 16 * it;
                        cur_tap[it] = tap;
                        cur_m[it] = mk[p + (tap / 5 - 2) * 9 + (tap % 5 - 2)];
                    }
                    any |= cur_m[it];
                }
                if (!__ballot(any != 0u)) break;
                float4 wa[LITER], wb[LITER];
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    wa[it] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    wb[it] = wa[it];
                    if (cur_m[it]) {
                        const int c = __builtin_ctz(cur_m[it]);
                        const float4* tp = reinterpret_cast<const float4*>(fa.table + ((size_t)(c * 25 + cur_tap[it]) * 128 + c8 * 8));
                        wa[it] = tp[0];
                        wb[it] = tp[1];
                    }
                }
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    if (cur_m[it]) {
                        acc[it][0] += wa[it].x; acc[it][1] += wa[it].y; acc[it][2] += wa[it].z; acc[it][3] += wa[it].w;
                        acc[it][4] += wb[it].x; acc[it][5] += wb[it].y; acc[it][6] += wb[it].z; acc[it][7] += wb[it].w;
                        cur_m[it] &= cur_m[it] - 1u;
                    }
                }
            }
        };
        auto first_end = [&]() {                              // ReLU, c8 split, pack (see write_x)
#pragma unroll
            for (int it = 0; it < LITER; ++it) {
                float r[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] = acc[it][j] > 0.0f ? acc[it][j] : 0.0f;
                const cf8::Split4 s0 = cf8::split4(r), s1 = cf8::split4(r + 4);
                struct alignas(16) H8 { Quad<_Float16> a, b; };
                v[0][it] = __builtin_bit_cast(uint4, H8{s0.hi, s1.hi});
                v[1][it] = make_uint4(s0.l8, s1.l8, s0.h8, s1.h8);
            }
        };
        if (FIRST) {
            planes_prefetch(t);
            first_begin();
            if (t + stride < n_boards) planes_prefetch(t + stride);
            first_rounds(25 * 32);
            first_end();
        } else {
            tile_load<_Float16, C, 1, 2, CTHR>(xh, reinterpret_cast<const _Float16*>(xc), t, n_boards, ctid, v);
        }
        write_x(ctid);
        zero_rows_write<C, 1, 2, CTHR>(X, ctid);
        zero_rows_write<C, 1, 2, CTHR>(Y, ctid);
        if (ctid < C) {
            reinterpret_cast<float*>(lds + BIAS_OFF)[ctid] = b1[ctid];
            reinterpret_cast<float*>(lds + BIAS_OFF)[C + ctid] = b2[ctid];
        }
        int t_prev = -1;
#ifdef CZ_RB_STAMPS
        int it_no = 0;
#endif
        for (;;) {
#ifdef CZ_RB_STAMPS
            const bool stamp_on = blockIdx.x == 5 && ctid == 0 && it_no++ == 40;
#endif
            RB_STAMP(16);
            __syncthreads();                                   // A_k: X holds board t
            RB_STAMP(17);
            const int tn = t + stride;
            const bool has_next = tn < n_boards;
            int ct2 = ctid;
            asm volatile("" : "+v"(ct2));                      // keep address arithmetic inside the loop (registers)
            if (FIRST) {
                if (has_next) {                                // first part of the next board's input layer, under K loop 1
                    __builtin_amdgcn_s_setprio(CZ_FIRST_PRIO);
                    first_begin();                             // (board tn: its planes were fetched a window ago)
                    RB_STAMP(24);
                    if (tn + stride < n_boards) planes_prefetch(tn + stride);
                    RB_STAMP(25);
                    first_rounds(fa.w1_rounds);
                    __builtin_amdgcn_s_setprio(0);
                }
            } else if (has_next) {
                tile_load<_Float16, C, 1, 2, CTHR>(xh, reinterpret_cast<const _Float16*>(xc), tn, n_boards, ct2, v);
            }
            RB_STAMP(18);
            __syncthreads();                                   // B_k: staging holds board t_prev; X is free
            RB_STAMP(19);
            if (t_prev >= 0) CZ_STORE_BOARD(t_prev, ct2);
            RB_STAMP(20);
            if (has_next) {
                if (FIRST) {
                    __builtin_amdgcn_s_setprio(CZ_FIRST_PRIO);
                    first_rounds(25 * 32);
                    RB_STAMP(21);
                    first_end();
                    __builtin_amdgcn_s_setprio(0);
                }
                RB_STAMP(22);
                write_x(ct2);
            }
            RB_STAMP(23);
            t_prev = t;
            if (!has_next) break;
            t = tn;
        }
        __syncthreads();                                       // E0: the staging image is free (the store above is done)
        __syncthreads();                                       // E1: the last board is staged
        CZ_STORE_BOARD(t_prev, ctid);
#undef CZ_STORE_BOARD
        return;
    }

    // ---- matrix waves ----
    const int kb = lane >> 5, ln = lane & 31;
    const c8k::Filter flt1 = c8k::make_filter(w1p, wave, lane), flt2 = c8k::make_filter(w2p, wave, lane);
    const float* bias1 = reinterpret_cast<const float*>(lds + BIAS_OFF);
    const float* bias2 = bias1 + C;
    f32x16 acc[NT], prev[NT];
    // c6: the exponents of the images the two convolutions read (X: not for the fused input layer's c8 image)
    const int k_x = C6 && !FIRST ? __builtin_amdgcn_readfirstlane(pack_ints(w1p)[2]) : 0;
    const int k_y = C6 ? __builtin_amdgcn_readfirstlane(pack_ints(w2p)[2]) : 0;
    rb8::Shadow shd{lds, prev, wave, kb, ln};
    bool have_prev = false;
#ifdef CZ_RB_STAMPS
    int it_no = 0;
#endif
    for (;;) {
#ifdef CZ_RB_STAMPS
        const bool stamp_on = blockIdx.x == 5 && tid == 0 && it_no++ == 40;
#endif
        RB_STAMP(0);
        __syncthreads();                                       // A_k
        RB_STAMP(1);
        const bool has_next = t + stride < n_boards;
        // K loop 1 on X, accumulators starting at b1
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bv = *reinterpret_cast<const float4*>(bias1 + wave * 32 + g * 8 + kb * 4);
#pragma unroll
            for (int p = 0; p < NT; ++p) {
                acc[p][g * 4 + 0] = bv.x; acc[p][g * 4 + 1] = bv.y; acc[p][g * 4 + 2] = bv.z; acc[p][g * 4 + 3] = bv.w;
            }
        }
        __builtin_amdgcn_s_setprio(3);
        constexpr int F1 = C6 && !FIRST ? 1 : 0;              // (the fused input layer hands over a c8 image)
        if (have_prev) c8k::kloop<NT, rb8::Shadow&, 0, false, 128, F1>(X, c8k::Image{0, ZROW, PART}, flt1, lane, acc, 127 + k_x - cf8::X_LO_SHIFT, 127 + k_x, shd);
        else c8k::kloop<NT, c8k::NoShadow, 0, false, 128, F1>(X, c8k::Image{0, ZROW, PART}, flt1, lane, acc, 127 + k_x - cf8::X_LO_SHIFT, 127 + k_x);
        __builtin_amdgcn_s_setprio(0);
        RB_STAMP(2);
        int ln2 = ln, kb2 = kb;
        asm volatile("" : "+v"(ln2), "+v"(kb2));
        // epilogue 1: relu(acc) -> c8 triple -> Y; the freed accumulators restart at b2 + skip (this lane's own elements of X)
        if (C6) {
            // c6: the f16 quads go out per lane as before; the two bf6 pieces of a pixel's 32 channels need the other
            // lane half's 16 values: tiles 0 and 1 trade halves (one v_permlane32_swap per register -- the lower lanes end
            // up with tile 0's pixels, the upper ones with tile 1's), tile 2 trades with itself (lower lanes store)
            const float s_hi = __builtin_ldexpf(1.0f, k_y), s_lo = __builtin_ldexpf(1.0f, k_y - cf8::X_LO_SHIFT);
            const float s_skip = __builtin_ldexpf(1.0f, k_x - cf8::X_LO_SHIFT);
            f32x16 lo[NT];
#pragma unroll
            for (int p = 0; p < NT; ++p) {
                const int q = p * 32 + ln2;
                const int row = q < 90 ? q : 89;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = wave * 32 + g * 8 + kb2 * 4;
                    const int off = row * RB + (((ch >> 3) ^ (row & 15)) << 4) + (ch & 7) * 2;
                    Quad<_Float16> hq;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float r = acc[p][g * 4 + i] > 0.0f ? acc[p][g * 4 + i] : 0.0f;
                        hq.e[i] = (_Float16)r;
                        acc[p][g * 4 + i] = r;
                        lo[p][g * 4 + i] = r - (float)hq.e[i];
                    }
                    if (q < 90) *reinterpret_cast<Quad<_Float16>*>(Y + off) = hq;
                }
            }
#pragma unroll
            for (int pp = 0; pp < 2; ++pp) {                   // pair (0, 1), then tile 2 with itself
                const int pa = pp == 0 ? 0 : 2, pb = pp == 0 ? 1 : 2;
                f32x16 av, bv, al, bl;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const auto sv = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[pa][r]), __float_as_uint(acc[pb][r]), false, false);
                    const auto sl = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo[pa][r]), __float_as_uint(lo[pb][r]), false, false);
                    av[r] = __uint_as_float(sv[0]); bv[r] = __uint_as_float(sv[1]);
                    al[r] = __uint_as_float(sl[0]); bl[r] = __uint_as_float(sl[1]);
                }
                const u32x6 pl = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(al, bl, s_lo);
                const u32x6 pv = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(av, bv, s_hi);
                const int q = pp == 0 ? kb2 * 32 + ln2 : 64 + ln2;
                if (pp == 0 || (kb2 == 0 && q < 90)) {
                    unsigned char* d0 = Y + PART + c6_lds_off(q, c6_chunk(0, wave));
                    unsigned char* t0 = Y + PART + c6_lds_off(q, c6_chunk(0, wave) + 1);
                    unsigned char* d1 = Y + PART + c6_lds_off(q, c6_chunk(1, wave));
                    unsigned char* t1 = Y + PART + c6_lds_off(q, c6_chunk(1, wave) + 1);
                    *reinterpret_cast<uint4*>(d0) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
                    *reinterpret_cast<uint2*>(t0) = make_uint2(pl[4], pl[5]);
                    *reinterpret_cast<uint4*>(d1) = make_uint4(pv[0], pv[1], pv[2], pv[3]);
                    *reinterpret_cast<uint2*>(t1) = make_uint2(pv[4], pv[5]);
                }
            }
            // the accumulators restart at b2 + skip: this lane's channels of X (f16 quads + its elements of the lo piece)
#pragma unroll
            for (int p = 0; p < NT; ++p) {
                const int q = p * 32 + ln2;
                const int row = q < 90 ? q : 89;
                f32x32 xl;
                if (!FIRST) {
                    const uint4 hd4 = *reinterpret_cast<const uint4*>(X + PART + c6_lds_off(row, c6_chunk(0, wave)));
                    const uint2 tl2 = *reinterpret_cast<const uint2*>(X + PART + c6_lds_off(row, c6_chunk(0, wave) + 1));
                    // the upper lane half wants the odd elements: it shifts the piece down by one element (6 bits), so that
                    // every lane reads element 2 r for its register r  (a select between xl[2 r] and xl[2 r + 1] is
                    // turned into a variable vector index by the compiler: 31 v_cndmask per element)
                    const uint32_t wv[7] = {hd4.x, hd4.y, hd4.z, hd4.w, tl2.x, tl2.y, 0u};
                    const uint32_t sh6 = (uint32_t)kb2 * 6u;
                    u32x6 pc;
#pragma unroll
                    for (int w = 0; w < 6; ++w) pc[w] = __builtin_amdgcn_alignbit(wv[w + 1], wv[w], sh6);
                    xl = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(pc, s_skip);
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = wave * 32 + g * 8 + kb2 * 4;
                    const int off = row * RB + (((ch >> 3) ^ (row & 15)) << 4) + (ch & 7) * 2;
                    const float4 bv4 = *reinterpret_cast<const float4*>(bias2 + ch);
                    float vv[4] = {bv4.x, bv4.y, bv4.z, bv4.w};
                    const Quad<_Float16> xq = *reinterpret_cast<const Quad<_Float16>*>(X + off);
                    if (FIRST) {
                        const int off_lo = PART + row * RB + (ch & 15) + (((ch >> 4) ^ (row & 15)) << 4);
                        cf8::add_pair4(vv, xq, *reinterpret_cast<const uint32_t*>(X + off_lo));
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int r = g * 4 + i;
                            vv[i] += (float)xq.e[i] + xl[2 * r];
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[p][g * 4 + i] = vv[i];
                }
            }
        } else {
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int q = p * 32 + ln2;
            const int row = q < 90 ? q : 89;                   // (padding lanes compute on row 89 and store nothing)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = wave * 32 + g * 8 + kb2 * 4;
                const int off = row * RB + (((ch >> 3) ^ (row & 15)) << 4) + (ch & 7) * 2;
                const int off_lo = PART + row * RB + (ch & 15) + (((ch >> 4) ^ (row & 15)) << 4);
                const int off_hi = PART + row * RB + (ch & 15) + (((8 + (ch >> 4)) ^ (row & 15)) << 4);
                float r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = acc[p][g * 4 + i] > 0.0f ? acc[p][g * 4 + i] : 0.0f;
                const cf8::Split4 o = cf8::split4(r);
                if (q < 90) {
                    *reinterpret_cast<Quad<_Float16>*>(Y + off) = o.hi;
                    *reinterpret_cast<uint32_t*>(Y + off_lo) = o.l8;
                    *reinterpret_cast<uint32_t*>(Y + off_hi) = o.h8;
                }
                const float4 bv = *reinterpret_cast<const float4*>(bias2 + ch);
                float vv[4] = {bv.x, bv.y, bv.z, bv.w};
                cf8::add_pair4(vv, *reinterpret_cast<const Quad<_Float16>*>(X + off), *reinterpret_cast<const uint32_t*>(X + off_lo));
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[p][g * 4 + i] = vv[i];
            }
        }
        }
        RB_STAMP(3);
        __syncthreads();                                       // B_k: Y complete, X and the previous staging contents free
        RB_STAMP(4);
        __builtin_amdgcn_s_setprio(3);
        c8k::kloop<NT, c8k::NoShadow, 0, false, 128, C6 ? 1 : 0>(Y, c8k::Image{0, ZROW, PART}, flt2, lane, acc, 127 + k_y - cf8::X_LO_SHIFT, 127 + k_y);
        __builtin_amdgcn_s_setprio(0);
        RB_STAMP(5);
#pragma unroll
        for (int p = 0; p < NT; ++p) prev[p] = acc[p];
        have_prev = true;
        if (!has_next) break;
        t += stride;
    }
    // the last board's second epilogue, not overlapped (once the copy waves have let go of the staging image)
    __syncthreads();                                           // E0
#pragma unroll
    for (int p = 0; p < NT; ++p)
#pragma unroll
        for (int g = 0; g < 4; ++g) shd.unit(prev[p], p * 32 + ln, g);
    __syncthreads();                                           // E1
}

}  // namespace
