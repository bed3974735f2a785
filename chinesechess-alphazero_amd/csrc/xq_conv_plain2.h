// xq_conv_plain2.h -- part of xq_conv.hip's translation unit; do not compile it into a second one: the unit's device code is
// compared kernel by kernel when text moves between these headers (EXPERIMENTS.md, "the convolution unit's text in headers"), and
// the search unit's kernels changed by 0.4-1.7 % when part of that unit was compiled alone.
//
// Kernel 2p: k_tower_plain2, a chain of residual blocks on plain 2-byte operands, a pair of boards per workgroup (pl::MAX_BLOCKS).
#pragma once
#include "xq_conv_kloop.h"

namespace {

// ---- kernel 2p: a CHAIN of residual blocks on plain 2-byte operands (256 filters: the `deep` 20 x 256 fp16 tower) ---------------
// k_resblock<E, 256, 1, 1, false, 2> keeps X | Y | a staging image and sends every block's result through the copy waves to HBM and
// back.  Here a workgroup takes a PAIR of boards through ALL blocks of the tower, HBM sees a board at the chain's entry and exit.
// What bounds the chain is energy per board (EXPERIMENTS Part III): per board and convolution 1.18 MB of packed filter come from
// L2 into the CU, and a filter fragment feeding SIX pixel tiles (two boards) instead of three halves that stream per board at the
// same LDS reads per MFMA.  Two boards with X | Y each do not fit 160 KB; they do with ONE image per board: after K loop 1
// (barrier: every wave has read all of X) a lane moves its own skip values out of X (a lane reads and writes only its own 8
// bytes) and writes relu(conv1 + b1) over them -- X now IS Y --, and epilogue 2 writes relu(conv2 + b2 + skip) to the same 8
// bytes again, which is block b + 1's input.  192 accumulator + 96 skip registers per wave: four matrix waves, no copy waves, one
// wave per SIMD (512 registers); the matrix waves fetch and store the pair themselves, once per chain.  K loop
// (conv_kloop<E, 256, 2, 1, 2>) and epilogue arithmetic are k_resblock's, per accumulator tile in the same order: bit-identical
// to ch.n launches of k_resblock (BASELINE configs[4]; reference tower agent/model.py:41-43).
namespace pl {
constexpr int MAX_BLOCKS = 24;
}  // namespace pl

template <typename E, int C, int CTW>
__global__ __launch_bounds__(C / 32 / CTW * 64, 1) void k_tower_plain2(
    const E* __restrict__ xh, BlockChain<pl::MAX_BLOCKS> ch, E* __restrict__ yh, int n_boards, const int32_t* __restrict__ n_dev)
{
    n_boards = nn_live_boards(n_boards, n_dev);
    typedef Geom<C, 2, 1> G;
    constexpr int NT = G::NT, NTHR = C / 32 / CTW * 64;
    constexpr int LITER = (G::CHUNKS + NTHR - 1) / NTHR;
    // X: the pair's image.  SK: the FIRST board's skip values while its intermediate activation sits in X (the second board's wait
    // in registers: 48 -- all 96 in registers left no room beside 192 accumulators and the K loop's rings: half of them spilled)
    __shared__ __attribute__((aligned(16))) unsigned char lds[G::REGION + 90 * G::RB];
    unsigned char* X = lds;
    unsigned char* SK = lds + G::REGION;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NB = ch.n;
    const int n_pairs = (n_boards + 1) / 2;
    const int wg = wave * CTW;                                 // first channel tile of this wave
    const int kb = lane >> 5, ln = lane & 31;
    zero_rows_write<C, 2, 1, NTHR>(X, tid);
    for (int t = blockIdx.x; t < n_pairs; t += gridDim.x) {
        {
            // global -> LDS image, 16 bytes per lane per step in flights of eight (a missing second board: zeros)
            typedef c8k::u32x4 u4;
            const u4* src = reinterpret_cast<const u4*>(xh + (size_t)2 * t * 90 * C);
            const int have = (n_boards - 2 * t < 2 ? n_boards - 2 * t : 2) * 90 * G::CPR;
#pragma unroll
            for (int it0 = 0; it0 < LITER; it0 += 8) {
                u4 v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int i = (it0 + j) * NTHR + tid;
                    v[j] = u4{0u, 0u, 0u, 0u};
                    if (it0 + j < LITER && i < have) v[j] = src[i];
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int i = (it0 + j) * NTHR + tid;
                    if (it0 + j < LITER && i < G::CHUNKS) {
                        const int row = i / G::CPR, chn = i % G::CPR;
                        *reinterpret_cast<u4*>(X + row * G::RB + ((chn ^ (row & G::SWZ)) << 4)) = v[j];
                    }
                }
            }
        }
        __syncthreads();                                       // A: X holds the pair
        for (int blk = 0; blk < NB; ++blk) {
            const uint4* wq1 = reinterpret_cast<const uint4*>(ch.w1[blk]) + wg * 64 + lane;
            const uint4* wq2 = reinterpret_cast<const uint4*>(ch.w2[blk]) + wg * 64 + lane;
            const float* b1 = ch.b1[blk];
            const float* b2 = ch.b2[blk];
            f32x16 acc[CTW * NT];
            c8k::u32x2 skip[CTW * 3][4];          // (packed: four 2-byte values in two registers)
            f32x4 bq[CTW][4];
            // the biases of this wave's channels: all eight loads in flight across the barrier, materialised once (left to the
            // compiler there was one load and one vmcnt(0) per 8-byte store: 48 L2 round trips in a row per epilogue)
            auto bias_request = [&](const float* bp) {
#pragma unroll
                for (int c = 0; c < CTW; ++c)
#pragma unroll
                    for (int g = 0; g < 4; ++g) bq[c][g] = *reinterpret_cast<const f32x4*>(bp + (wg + c) * 32 + g * 8 + kb * 4);
            };
            auto bias_pin = [&]() {
#pragma unroll
                for (int c = 0; c < CTW; ++c)
#pragma unroll
                    for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(bq[c][g]));
            };
            __builtin_amdgcn_s_setprio(3);
            conv_kloop<E, C, 2, 1, CTW>(X, wq1, lane, acc);
            __builtin_amdgcn_s_setprio(0);
            bias_request(b1);
            __syncthreads();                                   // K1: every wave has read X
            bias_pin();
            int ln2 = ln, kb2 = kb;
            asm volatile("" : "+v"(ln2), "+v"(kb2));
            // epilogue 1: skip <- X, X <- relu(acc + b1)   (this lane's own 8 bytes)
#pragma unroll
            for (int cp = 0; cp < CTW * NT; ++cp) {
                const int p = cp % NT, c = cp / NT;
                const int q = (p % 3) * 32 + ln2;
                const int row = (p / 3) * 90 + q;
                if (q < 90) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int chn = (wg + c) * 32 + g * 8 + kb2 * 4;
                        const f32x4 bv = bq[c][g];
                        const float vv[4] = {acc[cp][g * 4 + 0] + bv[0], acc[cp][g * 4 + 1] + bv[1], acc[cp][g * 4 + 2] + bv[2],
                                             acc[cp][g * 4 + 3] + bv[3]};
                        const int off = row * G::RB + (((chn >> 3) ^ (row & G::SWZ)) << 4) + (chn & 7) * 2;
                        const c8k::u32x2 sk = *reinterpret_cast<const c8k::u32x2*>(X + off);
                        if (p < 3) *reinterpret_cast<c8k::u32x2*>(SK + off) = sk;
                        else skip[c * 3 + p - 3][g] = sk;
                        Quad<E> hi;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float r = vv[i] > 0.0f ? vv[i] : 0.0f;
                            hi.e[i] = (E)r;
                        }
                        *reinterpret_cast<Quad<E>*>(X + off) = hi;
                    }
                }
            }
            __syncthreads();                                   // B: X holds the intermediate activation
            __builtin_amdgcn_s_setprio(3);
            conv_kloop<E, C, 2, 1, CTW>(X, wq2, lane, acc);
            __builtin_amdgcn_s_setprio(0);
            bias_request(b2);
            __syncthreads();                                   // K2: every wave has read it
            bias_pin();
            asm volatile("" : "+v"(ln2), "+v"(kb2));
            // epilogue 2: X <- relu(acc + b2 + skip)
#pragma unroll
            for (int cp = 0; cp < CTW * NT; ++cp) {
                const int p = cp % NT, c = cp / NT;
                const int q = (p % 3) * 32 + ln2;
                const int row = (p / 3) * 90 + q;
                if (q < 90) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int chn = (wg + c) * 32 + g * 8 + kb2 * 4;
                        const f32x4 bv = bq[c][g];
                        const int off = row * G::RB + (((chn >> 3) ^ (row & G::SWZ)) << 4) + (chn & 7) * 2;
                        float vv[4] = {acc[cp][g * 4 + 0] + bv[0], acc[cp][g * 4 + 1] + bv[1], acc[cp][g * 4 + 2] + bv[2],
                                       acc[cp][g * 4 + 3] + bv[3]};
                        const c8k::u32x2 sk = p < 3 ? *reinterpret_cast<const c8k::u32x2*>(SK + off) : skip[c * 3 + p - 3][g];
                        const Quad<E> sh = __builtin_bit_cast(Quad<E>, sk);
                        Quad<E> o;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            vv[i] += (float)sh.e[i];
                            vv[i] = vv[i] > 0.0f ? vv[i] : 0.0f;
                            o.e[i] = (E)vv[i];
                        }
                        *reinterpret_cast<Quad<E>*>(X + off) = o;
                    }
                }
            }
            __syncthreads();                                   // C: the block's result is in X
        }
        // the chain's result to HBM
        const int valid = (n_boards - 2 * t < 2 ? n_boards - 2 * t : 2) * 90 * G::CPR;
        c8k::u32x4* dst = reinterpret_cast<c8k::u32x4*>(yh + (size_t)2 * t * 90 * C);
#pragma unroll
        for (int it = 0; it < LITER; ++it) {
            const int i = it * NTHR + tid;
            if (!((it + 1) * NTHR <= G::CHUNKS || i < G::CHUNKS) || i >= valid) continue;
            const int row = i / G::CPR, chn = i % G::CPR;
            dst[i] = *reinterpret_cast<const c8k::u32x4*>(X + row * G::RB + ((chn ^ (row & G::SWZ)) << 4));
        }
        __syncthreads();                                       // X may take the next pair
    }
}

}  // namespace
