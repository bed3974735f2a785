// xq_conv_block.h -- part of xq_conv.hip's translation unit; do not compile it into a second one: the unit's device code is
// compared kernel by kernel when text moves between these headers (EXPERIMENTS.md, "the convolution unit's text in headers"), and
// the search unit's kernels changed by 0.4-1.7 % when part of that unit was compiled alone.
//
// Kernel 2: k_resblock, a whole residual block per launch on matrix waves + copy waves (RB_COPY_THREADS), optionally with the two
// 1x1 head convolutions in its store pass.
#pragma once
#include "xq_conv_kloop.h"

namespace {

// ---- kernel 2: a whole residual block per launch, wave-specialised ---------------------------------------------------
// y = relu(conv2(relu(conv1(x) + b1)) + b2 + x) for P boards at a time per workgroup, persistent over boards.
// The intermediate activation never leaves LDS (it is written straight into a second operand image), the skip
// operand is read back from the first image, and HBM sees one read of x and one write of y per block instead of
// 2 reads + 1 skip read + 2 writes.  Waves 0..CT-1 ("matrix waves", 32 output channels each) only run K loops and the
// two register-level epilogues; 4 more waves ("copy waves") own all global traffic: they fetch the NEXT boards into
// registers while the matrix waves work (their vmcnt is their own, so nothing in the K loop waits for it), drop them
// into the X image the moment the matrix waves are done with it, and stream the PREVIOUS boards' staged result out
// (16 bytes per lane, re-split into hi/lo in split mode) under the next K loop.
//   LDS: X image | Y image | staging (fp32 in split mode, final 2-byte values otherwise); one workgroup per CU:
//     128 filters split  (P = 1): 46.6 + 46.6 + 46.1 KB, 4 + 4 waves      128 filters plain (P = 2): the same bytes
//     256 filters plain  (P = 1): 46.6 + 46.6 + 46.1 KB, 8 + 4 waves      192 filters plain (P = 1): 34.9 + 34.9 + 34.6
//     (192 / 256 filters with split operands do not fit: those run one k_conv3x3 per convolution)
//   barriers per tile: A (X ready) .. K1 .. epi1 -> Y .. B (Y ready) .. K2 .. epi2 -> staging .. C (staged, X free)
constexpr int RB_COPY_THREADS = 256;

template <typename E, int C, int PARTS, int P, bool HEADS = false, int CTW = 1>
__global__ __launch_bounds__((C / 32 / CTW + 4) * 64, (C / 32 / CTW + 4 + 3) / 4) void k_resblock(
    const E* __restrict__ xh, const E* __restrict__ xl, const E* __restrict__ w1p, const float* __restrict__ b1,
    const E* __restrict__ w2p, const float* __restrict__ b2, E* __restrict__ yh, E* __restrict__ yl,
    float* __restrict__ yf, int n_boards, HeadArgs hd, const int32_t* __restrict__ n_dev)
{
    static_assert(!HEADS || (PARTS == 2 && C / 8 == 16), "fused heads: split operands, 128 filters");
    n_boards = nn_live_boards(n_boards, n_dev);
    typedef Geom<C, P, PARTS> G;
    constexpr int NT = G::NT, CT = G::CT / CTW, CTHR = RB_COPY_THREADS;      // CT: matrix waves, CTW channel tiles each
    static_assert(G::CT % CTW == 0, "channel tiles per wave must divide the channel tiles");
    constexpr int SROW = PARTS == 2 ? C * 4 : C * 2;   // staging row (one pixel): fp32, or the final 2-byte values
    constexpr int PIECES = P * 90 * (C / 8);           // 8-channel output pieces per tile
    constexpr int EITER = (PIECES + CTHR - 1) / CTHR;
    constexpr int LITER = (G::CHUNKS + CTHR - 1) / CTHR;
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * G::REGION + P * 90 * SROW];
    unsigned char* X = lds;
    unsigned char* Y = lds + G::REGION;
    unsigned char* S = lds + 2 * G::REGION;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool copy_role = wave >= CT;
    const int n_tiles = (n_boards + P - 1) / P;
    int t = blockIdx.x;                                 // tile = P consecutive boards
    if (t >= n_tiles) return;
    const int stride = gridDim.x;
    // staging offset of channels ch..ch+3 of tile pixel qq
    auto stage_off = [&](int qq, int ch) {
        if (PARTS == 2) return qq * SROW + ((((ch >> 2) & ~7) | (((ch >> 2) ^ qq) & 7)) << 4);
        return qq * SROW + ((((ch >> 3) ^ (qq & G::SWZ))) << 4) + (ch & 7) * 2;
    };

    if (copy_role) {
        const int ctid = tid - CT * 64;
        uint4 v[PARTS][LITER];
        tile_load<E, C, P, PARTS, CTHR>(xh, xl, t * P, n_boards, ctid, v);
        tile_write<C, P, PARTS, CTHR>(X, ctid, v);
        zero_rows_write<C, P, PARTS, CTHR>(X, ctid);
        zero_rows_write<C, P, PARTS, CTHR>(Y, ctid);
        int t_prev = -1;
        float hw[HEADS ? 6 : 1][8];                            // this thread's slice of the head filters (c8 is fixed)
        if (HEADS) {
#pragma unroll
            for (int o = 0; o < 6; ++o)
#pragma unroll
                for (int k = 0; k < 8; ++k) hw[o][k] = hd.w[o * C + (ctid % (C / 8)) * 8 + k];
        }
        for (;;) {
            __syncthreads();                                   // A: X holds tile t
            const int tn = t + stride;
            const bool has_next = tn < n_tiles;
            int ct2 = ctid;
            asm volatile("" : "+v"(ct2));                      // keep address arithmetic inside the loop (registers)
            if (has_next) tile_load<E, C, P, PARTS, CTHR>(xh, xl, tn * P, n_boards, ct2, v);
            // stream out the previous tile (staged, already ReLU'd) while the matrix waves run K1
            auto store_tile = [&](int to) {
                const size_t ebase = (size_t)to * P * 90 * C;
                const int valid = (n_boards - to * P < P ? n_boards - to * P : P) * 90 * (C / 8);
#pragma unroll
                for (int it = 0; it < EITER; ++it) {
                    const int i = it * CTHR + ct2;
                    if (!((it + 1) * CTHR <= PIECES || i < PIECES) || i >= valid) continue;
                    const int qq = i / (C / 8), c8 = i % (C / 8);
                    if (PARTS == 2) {
                        const float4 f0 = *reinterpret_cast<const float4*>(S + stage_off(qq, c8 * 8));
                        const float4 f1 = *reinterpret_cast<const float4*>(S + stage_off(qq, c8 * 8 + 4));
                        const float r[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                        if (HEADS) {
                            // 16 consecutive lanes hold the 128 channels of one pixel: partial dot products, then a
                            // 16-lane butterfly; lane o of the group writes head output o
                            float hs[6];
#pragma unroll
                            for (int o = 0; o < 6; ++o) {
                                float a = 0.0f;
#pragma unroll
                                for (int k = 0; k < 8; ++k) a += r[k] * hw[o][k];
                                a = row16_sum(a);
                                hs[o] = a;
                            }
                            const int board = to * P + qq / 90, q = qq % 90;
#pragma unroll
                            for (int o = 0; o < 6; ++o)
                                if (c8 == o) {
                                    float v = hs[o] + hd.b[o];
                                    v = v > 0.0f ? v : 0.0f;
                                    if (o < hd.n_pol) hd.pol[(size_t)board * (hd.n_pol * 90) + o * 90 + q] = v;
                                    else hd.val[(size_t)board * ((6 - hd.n_pol) * 90) + (o - hd.n_pol) * 90 + q] = v;
                                }
                        } else if (yf) {
                            float4* o = reinterpret_cast<float4*>(yf + ebase) + 2 * i;
                            o[0] = f0;
                            o[1] = f1;
                        } else {
                            struct alignas(16) E8 { E e[8]; };
                            E8 hi, lo;
#pragma unroll
                            for (int k = 0; k < 8; ++k) {
                                hi.e[k] = (E)r[k];
                                lo.e[k] = (E)(r[k] - (float)hi.e[k]);
                            }
                            reinterpret_cast<uint4*>(yh + ebase)[i] = __builtin_bit_cast(uint4, hi);
                            reinterpret_cast<uint4*>(yl + ebase)[i] = __builtin_bit_cast(uint4, lo);
                        }
                    } else {
                        const uint4 f = *reinterpret_cast<const uint4*>(S + stage_off(qq, c8 * 8));
                        reinterpret_cast<uint4*>(yh + ebase)[i] = f;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            if (t_prev >= 0) store_tile(t_prev);
            __syncthreads();                                   // B
            __syncthreads();                                   // C: tile t is staged, X is free
            if (has_next) tile_write<C, P, PARTS, CTHR>(X, ct2, v);
            t_prev = t;
            if (!has_next) {
                store_tile(t);
                break;
            }
            t = tn;
        }
        return;
    }

    // ---- matrix waves ----
    const int wg = wave * CTW;                                 // first channel tile of this wave
    const uint4* wq1 = reinterpret_cast<const uint4*>(w1p) + wg * 64 + lane;
    const uint4* wq2 = reinterpret_cast<const uint4*>(w2p) + wg * 64 + lane;
    const int kb = lane >> 5, ln = lane & 31;
    for (;;) {
        __syncthreads();                                       // A
        const bool has_next = t + stride < n_tiles;
        f32x16 acc[CTW * NT];
        __builtin_amdgcn_s_setprio(3);
        conv_kloop<E, C, P, PARTS, CTW>(X, wq1, lane, acc);
        __builtin_amdgcn_s_setprio(0);
        // the biases of this wave's channels: all loads in flight at once, materialised once (round 6: left to the compiler there
        // was one load and one vmcnt(0) per 8-byte store -- 4 CTW NT L2 round trips in a row per epilogue, 7 % of the deep tower)
        f32x4 bq[CTW][4];
        auto bias_fetch = [&](const float* bp) {
#pragma unroll
            for (int c = 0; c < CTW; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) bq[c][g] = *reinterpret_cast<const f32x4*>(bp + (wg + c) * 32 + g * 8 + kb * 4);
#pragma unroll
            for (int c = 0; c < CTW; ++c)
#pragma unroll
                for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(bq[c][g]));
        };
        bias_fetch(b1);
        int ln2 = ln, kb2 = kb, gt2 = tid;
        asm volatile("" : "+v"(ln2), "+v"(kb2), "+v"(gt2));
        // epilogue 1: relu(acc + b1) -> (hi, lo) -> Y image (operand layout of the second convolution)
#pragma unroll
        for (int cp = 0; cp < CTW * NT; ++cp) {
            const int p = cp % NT, c = cp / NT;
            const int q = (p % 3) * 32 + ln2;
            const int row = (p / 3) * 90 + q;
            if (q < 90) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = (wg + c) * 32 + g * 8 + kb2 * 4;
                    const f32x4 bv = bq[c][g];
                    const float vv[4] = {acc[cp][g * 4 + 0] + bv[0], acc[cp][g * 4 + 1] + bv[1], acc[cp][g * 4 + 2] + bv[2],
                                         acc[cp][g * 4 + 3] + bv[3]};
                    const int off = row * G::RB + (((ch >> 3) ^ (row & G::SWZ)) << 4) + (ch & 7) * 2;
                    Quad<E> hi, lo;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float r = vv[i] > 0.0f ? vv[i] : 0.0f;
                        hi.e[i] = (E)r;
                        lo.e[i] = (E)(r - (float)hi.e[i]);
                    }
                    *reinterpret_cast<Quad<E>*>(Y + off) = hi;
                    if (PARTS == 2) *reinterpret_cast<Quad<E>*>(Y + G::PART_BYTES + off) = lo;
                }
            }
        }
        __syncthreads();                                       // B: Y complete
        __builtin_amdgcn_s_setprio(3);
        conv_kloop<E, C, P, PARTS, CTW>(Y, wq2, lane, acc);
        __builtin_amdgcn_s_setprio(0);
        bias_fetch(b2);
        asm volatile("" : "+v"(ln2), "+v"(kb2));
        // epilogue 2: relu(acc + b2 + x) -> staging
#pragma unroll
        for (int cp = 0; cp < CTW * NT; ++cp) {
            const int p = cp % NT, c = cp / NT;
            const int q = (p % 3) * 32 + ln2;
            const int row = (p / 3) * 90 + q;
            if (q < 90) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = (wg + c) * 32 + g * 8 + kb2 * 4;
                    const f32x4 bv = bq[c][g];
                    const int off = row * G::RB + (((ch >> 3) ^ (row & G::SWZ)) << 4) + (ch & 7) * 2;
                    const Quad<E> sh = *reinterpret_cast<const Quad<E>*>(X + off);
                    float vv[4] = {acc[cp][g * 4 + 0] + bv[0], acc[cp][g * 4 + 1] + bv[1], acc[cp][g * 4 + 2] + bv[2],
                                   acc[cp][g * 4 + 3] + bv[3]};
#pragma unroll
                    for (int i = 0; i < 4; ++i) vv[i] += (float)sh.e[i];
                    if (PARTS == 2) {
                        const Quad<E> sl = *reinterpret_cast<const Quad<E>*>(X + G::PART_BYTES + off);
#pragma unroll
                        for (int i = 0; i < 4; ++i) vv[i] += (float)sl.e[i];
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) vv[i] = vv[i] > 0.0f ? vv[i] : 0.0f;
                    if (PARTS == 2) {
                        *reinterpret_cast<float4*>(S + stage_off(row, ch)) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                    } else {
                        Quad<E> o;
#pragma unroll
                        for (int i = 0; i < 4; ++i) o.e[i] = (E)vv[i];
                        *reinterpret_cast<Quad<E>*>(S + stage_off(row, ch)) = o;
                    }
                }
            }
        }
        __syncthreads();                                       // C: staged; X may be replaced
        if (!has_next) break;
        t += stride;
    }
}

}  // namespace
