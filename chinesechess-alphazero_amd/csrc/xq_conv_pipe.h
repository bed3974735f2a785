// xq_conv_pipe.h -- part of xq_conv.hip's translation unit; do not compile it into a second one: the unit's device code is
// compared kernel by kernel when text moves between these headers (EXPERIMENTS.md, "the convolution unit's text in headers"), and
// the search unit's kernels changed by 0.4-1.7 % when part of that unit was compiled alone.
//
// Kernel 2b: k_resblock_pipe, the 128-filter residual block on operand pairs, software-pipelined over boards; FIRST: with the fused
// 5 x 5 input layer, whose algorithm is described here.
#pragma once
#include "xq_nn_common.h"

namespace {

// ---- kernel 2b: the residual block, software-pipelined over boards (128 filters, split operands) ------------------
// Same arithmetic as k_resblock (bit-identical results), different schedule: the second epilogue of board t-1
// (+ bias2 + skip, ReLU, re-split) runs in the SHADOW of board t's first K loop instead of between the K loops, and
// writes its result IN PLACE over the skip operand, in the operand layout -- so there is no fp32 staging buffer, no
// conversion in the copy waves, no hand-over of X between the roles, and two barriers per board instead of three.
//   LDS: three images (X even, X odd, Y) of 90 rows x 256 B per part, 16 zero rows shared by all of them, the two bias
//   vectors: 2 x (270 + 2 + 16) rows x 256 B + 1 KB = 148.5 KB.  Absolute row r of part q is byte (q * PSTR + r * 256).
//   matrix waves, board k (X = image k & 1):  A | K1(k) with epi2(k-1) in its shadow | epi1(k) -> Y | B | K2(k) | ...
//   copy waves:                               A | prefetch board k+1 (registers)     |             | B | drain out(k-1)
//                                                 from image (k-1) & 1 to HBM and refill the same chunks with board k+1
// The shadow work is cut into 12 units (pixel tile p x channel group g); K loop 1 is a rolled loop over 3 x (3 taps =
// 216 MFMA slots) and each pass retires the 4 units of one pixel tile, whose accumulators are then rotated out, so
// every register index in the loop body is static.
// FIRST: the block is the first of the tower and its input is the 5 x 5 input convolution of the feature planes
// (Conv2D(F, 5) -> BatchNorm -> ReLU, agent/model.py:36-39), computed HERE by the copy waves instead of by a kernel of
// its own.  The planes are one-hot -- a position has at most 32 pieces, 64 plane bits with the history planes -- so the
// layer is a gather: output pixel p, channel o = bias[o] + sum over the occupied squares q of p's 5 x 5 window of
// w[o][plane at q][tap].  A copy thread owns the 8 channels of its 16-byte chunk for 6 pixels (the chunks it writes into
// the X image anyway): 48 fp32 accumulators, ~55 weight loads of 32 bytes from an L2-resident table
// (table[plane][tap][128], 179 KB) per board, exact fp32 sums in a fixed order (bias, taps 0..24, planes ascending) --
// no MFMA, no second kernel, no 46 KB per board written and read back.  The work is split over the two windows a copy
// wave has per board (under K loop 1 and under K loop 2), since all waves meet at the barrier between them.

template <typename E, bool FIRST = false>
__global__ __launch_bounds__(512, 1) void k_resblock_pipe(
    const E* __restrict__ xh, const E* __restrict__ xl, const E* __restrict__ w1p, const float* __restrict__ b1,
    const E* __restrict__ w2p, const float* __restrict__ b2, E* __restrict__ yh, E* __restrict__ yl, int n_boards,
    const int32_t* __restrict__ n_dev, FirstArgs fa)
{
    using namespace pipe;
    constexpr int C = 128, CHUNKS = 90 * 16, CTHR = 256, LITER = (CHUNKS + CTHR - 1) / CTHR;
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_BYTES];
    n_boards = nn_live_boards(n_boards, n_dev);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = gridDim.x;
    int t = blockIdx.x;
    if (t >= n_boards) return;
    // chunk i of a board: row i / 16, chunk i % 16 -> LDS byte (image row base + row) * 256 + ((ch ^ (row & 15)) << 4)
    auto chunk_off = [&](int img, int i) {
        const int row = i >> 4, ch = i & 15;
        return (img * IMG_ROWS + row) * RB + ((ch ^ (row & 15)) << 4);
    };

    if (wave >= 4) {                                   // ---- copy waves ----
        const int ctid = tid - 256;
        uint4 v[2][LITER];
        auto fetch = [&](int board) {
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const uint4* src = reinterpret_cast<const uint4*>((part ? xl : xh) + (size_t)board * 90 * C);
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    const int i = it * CTHR + ctid;
                    v[part][it] = make_uint4(0, 0, 0, 0);
                    if ((it + 1) * CTHR <= CHUNKS || i < CHUNKS) v[part][it] = src[i];
                }
            }
        };
        auto put = [&](int img) {
#pragma unroll
            for (int part = 0; part < 2; ++part)
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    const int i = it * CTHR + ctid;
                    if ((it + 1) * CTHR <= CHUNKS || i < CHUNKS)
                        *reinterpret_cast<uint4*>(lds + part * PSTR + chunk_off(img, i)) = v[part][it];
                }
        };
        // result of `board` sits in image img (operand layout): to HBM; then the same chunks take the prefetched board
        auto drain = [&](int img, int board, bool refill) {
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                uint4* dst = reinterpret_cast<uint4*>((part ? yl : yh) + (size_t)board * 90 * C);
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    const int i = it * CTHR + ctid;
                    if (!((it + 1) * CTHR <= CHUNKS || i < CHUNKS)) continue;
                    unsigned char* a = lds + part * PSTR + chunk_off(img, i);
                    const uint4 o = *reinterpret_cast<const uint4*>(a);
                    if (refill) *reinterpret_cast<uint4*>(a) = v[part][it];
                    dst[i] = o;
                }
            }
        };
        // ---- FIRST: the input layer of board `board` into v[][] (the chunk layout put() / drain() write), in two halves ----
        // (planes_prefetch, first_begin and first_rounds exist a second time, statement for statement, in k_resblock_c8<FIRST>,
        //  csrc/xq_conv_block_c8.h: a change to one goes into the other; why they are not one definition: EXPERIMENTS.md)
        float acc[FIRST ? LITER : 1][8];
        uint32_t occ[FIRST ? LITER : 1], cur_m[FIRST ? LITER : 1];
        int cur_tap[FIRST ? LITER : 1];
        uint32_t* mk = reinterpret_cast<uint32_t*>(lds + MASK_OFF) + (wave - 4) * 96;     // this wave's own mask board
        const int c8 = ctid & 15, prow = ctid >> 4;            // chunk = channels 8 c8 .. 8 c8 + 7 of pixels prow + 16 it
        constexpr int PW = 12;                                 // plane words per lane: 32 planes x 90 bytes / 4 / 64 lanes
        uint32_t pw[FIRST ? PW : 1];
        auto planes_prefetch = [&](int board) {                // HBM -> registers, consumed by the next first_begin
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
            // the occupied planes of every square as a bit mask: handed in ready-made (fa.masks, cz_search_leaf_masks), or
            // built by each copy wave for itself (no barrier with the other copy waves: they share nothing)
            if (fa.masks) {
                mk[lane] = pw[0];
                if constexpr (FIRST) {
                    if (lane < 32) mk[64 + lane] = pw[1];
                }
            } else {
                mk[lane] = 0u;
                if (lane < 32) mk[64 + lane] = 0u;
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_wave_barrier();
                // (the board's plane words are already in registers: planes_prefetch ran a window earlier)
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
            // the occupied squares as one 90-bit set (wave-uniform): a pixel's occupied taps are five 5-bit windows of it
            const uint64_t occ_lo = __ballot(mk[lane] != 0u);
            const uint64_t occ_hi = __ballot(lane < 26 && mk[64 + (lane & 31)] != 0u);
            const float4 b0 = *reinterpret_cast<const float4*>(fa.in_bias + c8 * 8);
            const float4 b1v = *reinterpret_cast<const float4*>(fa.in_bias + c8 * 8 + 4);
#pragma unroll
            for (int it = 0; it < LITER; ++it) {
                acc[it][0] = b0.x; acc[it][1] = b0.y; acc[it][2] = b0.z; acc[it][3] = b0.w;
                acc[it][4] = b1v.x; acc[it][5] = b1v.y; acc[it][6] = b1v.z; acc[it][7] = b1v.w;
                // the taps of pixel `it` whose square is occupied, as a 25-bit set
                const int p = prow + 16 * it;
                const int py = p / 9, px = p - py * 9;
                uint32_t o = 0u;
                if (p < 90) {
#pragma unroll
                    for (int ky = 0; ky < 5; ++ky) {
                        const int r = py + ky - 2;
                        if ((unsigned)r < 10u) {
                            // the 9 squares of board row r, then columns px - 2 .. px + 2 (columns off the board shift in zeros)
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
        // One round = the next (tap, plane) term of each of the thread's six pixels: up to twelve 16-byte loads in flight,
        // then the adds.  A pixel's terms are taken taps ascending, planes ascending -- the summation order does not
        // depend on how the rounds fall.  Iterating over the terms a pixel HAS (9 on average, 25 at most) instead of over
        // the 25 taps halves the number of L2 round trips, which is all this loop costs.
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
        auto first_end = [&]() {                              // ReLU, split, pack: v[part][it] = chunk (pixel prow + 16 it, c8)
            struct alignas(16) E8 { E e[8]; };
#pragma unroll
            for (int it = 0; it < LITER; ++it) {
                E8 hi, lo;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float r = acc[it][j] > 0.0f ? acc[it][j] : 0.0f;
                    hi.e[j] = (E)r;
                    lo.e[j] = (E)(r - (float)hi.e[j]);
                }
                v[0][it] = __builtin_bit_cast(uint4, hi);
                v[1][it] = __builtin_bit_cast(uint4, lo);
            }
        };
        if (FIRST) {
            planes_prefetch(t);
            first_begin();
            if (t + stride < n_boards) planes_prefetch(t + stride);
            first_rounds(25 * 32);       // (to the end: a pixel has at most 25 taps x in_planes terms)
            first_end();
        } else {
            fetch(t);
        }
        put(0);
        for (int i = ctid; i < 16 * 16; i += CTHR) {          // the shared zero rows, both parts
            *reinterpret_cast<uint4*>(lds + ROW_Z * RB + i * 16) = make_uint4(0, 0, 0, 0);
            *reinterpret_cast<uint4*>(lds + PSTR + ROW_Z * RB + i * 16) = make_uint4(0, 0, 0, 0);
        }
        if (ctid < 128) {
            reinterpret_cast<float*>(lds + BIAS_OFF)[ctid] = b1[ctid];
            reinterpret_cast<float*>(lds + BIAS_OFF)[128 + ctid] = b2[ctid];
        }
        int k = 0, t_prev = -1;
        for (;;) {
            __syncthreads();                                   // A_k
            const int tn = t + stride;
            const bool has_next = tn < n_boards;
            if (FIRST) {
                if (has_next) {                                // first half of the next board's input layer, under K loop 1
                    first_begin();                             // (board tn: its planes were fetched a window ago)
                    if (tn + stride < n_boards) planes_prefetch(tn + stride);
                    first_rounds(fa.w1_rounds);
                }
            } else if (has_next) {
                fetch(tn);
            }
            __syncthreads();                                   // B_k: out(k-1) complete in image (k-1) & 1
            if (FIRST) {
                if (t_prev >= 0) drain((k - 1) & 1, t_prev, false);
                if (has_next) {                                // second half, under K loop 2; then into the free image
                    first_rounds(25 * 32);       // (to the end: a pixel has at most 25 taps x in_planes terms)
                    first_end();
                    put((k - 1) & 1);
                }
            } else {
                if (t_prev >= 0) drain((k - 1) & 1, t_prev, has_next);
                else if (has_next) put(1);
            }
            t_prev = t;
            if (!has_next) break;
            t = tn;
            ++k;
        }
        __syncthreads();                                       // E1: K2 of the last board done
        __syncthreads();                                       // E2: its epilogue 2 written in place
        drain(k & 1, t_prev, false);
        return;
    }

    // ---- matrix waves ----
    const uint4* wq1 = reinterpret_cast<const uint4*>(w1p) + wave * 64 + lane;
    const uint4* wq2 = reinterpret_cast<const uint4*>(w2p) + wave * 64 + lane;
    const int kb = lane >> 5, ln = lane & 31;
    f32x16 acc[NT], prev[NT];
    PipeShadow<E> shd;
    shd.lds = lds; shd.wave = wave; shd.kb = kb; shd.ln = ln;
    int k = 0;
    for (;;) {
        __syncthreads();                                       // A_k: X(k) in image k & 1
        const bool has_next = t + stride < n_boards;
        shd.prev_row_base = ((k - 1) & 1) * IMG_ROWS;
        __builtin_amdgcn_s_setprio(3);
        if (k > 0) pipe_kloop<E, true>(lds, (k & 1) * IMG_ROWS, wq1, lane, acc, prev, shd);
        else pipe_kloop<E, false>(lds, (k & 1) * IMG_ROWS, wq1, lane, acc, prev, shd);
        __builtin_amdgcn_s_setprio(0);
        int ln2 = ln, kb2 = kb;
        asm volatile("" : "+v"(ln2), "+v"(kb2));
        // epilogue 1: relu(acc + b1) -> (hi, lo) -> Y (image 2)
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int q = p * 32 + ln2;
            if (q < 90) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = wave * 32 + g * 8 + kb2 * 4;
                    const float4 bv = *reinterpret_cast<const float4*>(lds + BIAS_OFF + ch * 4);
                    const float vv[4] = {acc[p][g * 4 + 0] + bv.x, acc[p][g * 4 + 1] + bv.y, acc[p][g * 4 + 2] + bv.z,
                                         acc[p][g * 4 + 3] + bv.w};
                    Quad<E> hi, lo;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float r = vv[i] > 0.0f ? vv[i] : 0.0f;
                        hi.e[i] = (E)r;
                        lo.e[i] = (E)(r - (float)hi.e[i]);
                    }
                    const int off = (2 * IMG_ROWS + q) * RB + (((ch >> 3) ^ (q & 15)) << 4) + (ch & 7) * 2;
                    *reinterpret_cast<Quad<E>*>(lds + off) = hi;
                    *reinterpret_cast<Quad<E>*>(lds + PSTR + off) = lo;
                }
            }
        }
        __syncthreads();                                       // B_k: Y complete (and out(k-1), written during K1)
        __builtin_amdgcn_s_setprio(3);
        pipe_kloop<E, false>(lds, 2 * IMG_ROWS, wq2, lane, acc, prev, shd);
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int p = 0; p < NT; ++p) prev[p] = acc[p];
        if (!has_next) break;
        t += stride;
        ++k;
    }
    __syncthreads();                                           // E1
    shd.prev_row_base = (k & 1) * IMG_ROWS;                    // epilogue 2 of the last board, not overlapped
#pragma unroll
    for (int p = 0; p < NT; ++p)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            shd.whole(prev[p], p, g);
        }
    __syncthreads();                                           // E2
}

}  // namespace
