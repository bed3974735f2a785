// xq_conv_ip.h -- part of xq_conv.hip's translation unit; do not compile it into a second one: the unit's device code is
// compared kernel by kernel when text moves between these headers (EXPERIMENTS.md, "the convolution unit's text in headers"), and
// the search unit's kernels changed by 0.4-1.7 % when part of that unit was compiled alone.
//
// Kernels 2c: the two-image (in-place) residual blocks at 192 filters, k_resblock_ip on operand pairs and k_resblock_ip_c8 on the
// c8 / c6 arithmetic.
#pragma once
#include "xq_c8_kloop.h"
#include "xq_conv_kloop.h"

namespace {

// ---- kernel 2c: the residual block with split operands where three LDS images do not fit (192 filters) --------------
// The reference's deployed topology is 10 x 192 (configs/distribute.py:84-87, data/model/model_192x10_config.json).
// With split operands a 192-filter image is 90 rows x 384 B x 2 parts = 69 KB: X + Y + a staging image (k_resblock) or
// X even + X odd + Y (k_resblock_pipe) need 207 KB, the CU has 160.  This kernel keeps TWO images -- X and Y, 16 zero
// rows shared by both, the bias vectors: 152 KB -- and gives up the overlap that the third image buys:
//   matrix waves (6, 32 output channels each):  A | K1 on X | epi1 -> Y | B | K2 on Y | epi2: + b2 + skip, ReLU, re-split,
//                                               written IN PLACE over the skip operand in X | C |
//   copy waves (2):                             A | prefetch the next board into registers       | B | C | drain X to
//                                               HBM (16 B per lane, whole rows) and refill it with the prefetched board
// so HBM sees one read of x and one write of y per block (two launches of k_conv3x3 read x twice -- operand and skip --
// and round-trip the intermediate activation, with 8-byte scattered stores), and the matrix waves wait only for the
// drain + refill of one image (LDS <-> registers; the HBM latency of the prefetch is under the K loops).
// Same K loop (conv_kloop) and the same epilogue arithmetic in the same order as k_conv3x3: bit-identical to two
// cz_conv3x3 launches.  The last block of a tower writes fp32 (y_f32) straight from the accumulators' epilogue instead.
template <typename E, int C>
__global__ __launch_bounds__((C / 32) * 64 + ip::COPY_THREADS, 1) void k_resblock_ip(
    const E* __restrict__ xh, const E* __restrict__ xl, const E* __restrict__ w1p, const float* __restrict__ b1,
    const E* __restrict__ w2p, const float* __restrict__ b2, E* __restrict__ yh, E* __restrict__ yl,
    float* __restrict__ yf, int n_boards, const int32_t* __restrict__ n_dev)
{
    typedef Geom<C, 1, 2> G;
    constexpr int RB = G::RB, CPR = G::CPR, CT = G::CT, NT = 3;
    constexpr int PSTR = ip::ROWS * RB;                         // bytes per operand part
    constexpr int BIAS_OFF = 2 * PSTR;
    constexpr int CTHR = ip::COPY_THREADS, CHUNKS = 90 * CPR, LITER = (CHUNKS + CTHR - 1) / CTHR;
    __shared__ __attribute__((aligned(16))) unsigned char lds[BIAS_OFF + 2 * C * 4];
    static_assert(sizeof(lds) <= 160 * 1024, "two images + zero rows must fit the CU's LDS");
    n_boards = nn_live_boards(n_boards, n_dev);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = gridDim.x;
    int t = blockIdx.x;
    if (t >= n_boards) return;
    // chunk i of a board (row i / CPR, chunk i % CPR) in the X image
    auto chunk_off = [&](int i) {
        const int row = i / CPR, ch = i - row * CPR;
        return row * RB + ((ch ^ (row & G::SWZ)) << 4);
    };

    if (wave >= CT) {                                           // ---- copy waves ----
        const int ctid = tid - CT * 64;
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
        auto put = [&]() {
#pragma unroll
            for (int part = 0; part < 2; ++part)
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    const int i = it * CTHR + ctid;
                    if ((it + 1) * CTHR <= CHUNKS || i < CHUNKS)
                        *reinterpret_cast<uint4*>(lds + part * PSTR + chunk_off(i)) = v[part][it];
                }
        };
        // the block's result sits in X (operand layout): to HBM; the same chunks then take the prefetched board
        auto drain = [&](int board, bool refill) {
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                uint4* dst = reinterpret_cast<uint4*>((part ? yl : yh) + (size_t)board * 90 * C);
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    const int i = it * CTHR + ctid;
                    if (!((it + 1) * CTHR <= CHUNKS || i < CHUNKS)) continue;
                    unsigned char* a = lds + part * PSTR + chunk_off(i);
                    if (!yf) dst[i] = *reinterpret_cast<const uint4*>(a);
                    if (refill) *reinterpret_cast<uint4*>(a) = v[part][it];
                }
            }
        };
        fetch(t);
        put();
        for (int i = ctid; i < 16 * CPR; i += CTHR) {           // the shared zero rows, both parts
            *reinterpret_cast<uint4*>(lds + ip::ROW_Z * RB + i * 16) = make_uint4(0, 0, 0, 0);
            *reinterpret_cast<uint4*>(lds + PSTR + ip::ROW_Z * RB + i * 16) = make_uint4(0, 0, 0, 0);
        }
        for (int i = ctid; i < C; i += CTHR) {
            reinterpret_cast<float*>(lds + BIAS_OFF)[i] = b1[i];
            reinterpret_cast<float*>(lds + BIAS_OFF)[C + i] = b2[i];
        }
        for (;;) {
            __syncthreads();                                    // A: X holds board t
            const int tn = t + stride;
            const bool has_next = tn < n_boards;
            if (has_next) fetch(tn);
            __syncthreads();                                    // B: Y complete
            __syncthreads();                                    // C: the result is in X
            drain(t, has_next);
            if (!has_next) break;
            t = tn;
        }
        return;
    }

    // ---- matrix waves ----
    const uint4* wq1 = reinterpret_cast<const uint4*>(w1p) + wave * 64 + lane;
    const uint4* wq2 = reinterpret_cast<const uint4*>(w2p) + wave * 64 + lane;
    const int kb = lane >> 5, ln = lane & 31;
    const float* bias1 = reinterpret_cast<const float*>(lds + BIAS_OFF);
    const float* bias2 = bias1 + C;
    for (;;) {
        __syncthreads();                                        // A
        const bool has_next = t + stride < n_boards;
        f32x16 acc[NT];
        __builtin_amdgcn_s_setprio(3);
        conv_kloop<E, C, 1, 2>(lds, wq1, lane, acc, 0, ip::ROW_Z, PSTR);
        __builtin_amdgcn_s_setprio(0);
        int ln2 = ln, kb2 = kb;
        asm volatile("" : "+v"(ln2), "+v"(kb2));
        // epilogue 1: relu(acc + b1) -> (hi, lo) -> Y image (operand layout of the second convolution)
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int q = p * 32 + ln2;
            if (q < 90) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = wave * 32 + g * 8 + kb2 * 4;
                    const float4 bv = *reinterpret_cast<const float4*>(bias1 + ch);
                    const float vv[4] = {acc[p][g * 4 + 0] + bv.x, acc[p][g * 4 + 1] + bv.y, acc[p][g * 4 + 2] + bv.z,
                                         acc[p][g * 4 + 3] + bv.w};
                    Quad<E> hi, lo;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float r = vv[i] > 0.0f ? vv[i] : 0.0f;
                        hi.e[i] = (E)r;
                        lo.e[i] = (E)(r - (float)hi.e[i]);
                    }
                    const int off = (ip::ROW_Y + q) * RB + (((ch >> 3) ^ (q & G::SWZ)) << 4) + (ch & 7) * 2;
                    *reinterpret_cast<Quad<E>*>(lds + off) = hi;
                    *reinterpret_cast<Quad<E>*>(lds + PSTR + off) = lo;
                }
            }
        }
        __syncthreads();                                        // B: Y complete
        __builtin_amdgcn_s_setprio(3);
        conv_kloop<E, C, 1, 2>(lds, wq2, lane, acc, ip::ROW_Y, ip::ROW_Z, PSTR);
        __builtin_amdgcn_s_setprio(0);
        asm volatile("" : "+v"(ln2), "+v"(kb2));
        // epilogue 2: relu(acc + b2 + x) -> (hi, lo) in place over the skip operand (each lane reads and writes only its own
        // 8 bytes of each part), or fp32 straight to HBM for the last block of a tower
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int q = p * 32 + ln2;
            if (q < 90) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = wave * 32 + g * 8 + kb2 * 4;
                    const float4 bv = *reinterpret_cast<const float4*>(bias2 + ch);
                    const int off = q * RB + (((ch >> 3) ^ (q & G::SWZ)) << 4) + (ch & 7) * 2;
                    const Quad<E> sh = *reinterpret_cast<const Quad<E>*>(lds + off);
                    const Quad<E> sl = *reinterpret_cast<const Quad<E>*>(lds + PSTR + off);
                    float vv[4] = {acc[p][g * 4 + 0] + bv.x, acc[p][g * 4 + 1] + bv.y, acc[p][g * 4 + 2] + bv.z,
                                   acc[p][g * 4 + 3] + bv.w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) vv[i] += (float)sh.e[i];
#pragma unroll
                    for (int i = 0; i < 4; ++i) vv[i] += (float)sl.e[i];
#pragma unroll
                    for (int i = 0; i < 4; ++i) vv[i] = vv[i] > 0.0f ? vv[i] : 0.0f;
                    if (yf) {
                        *reinterpret_cast<float4*>(yf + ((size_t)t * 90 + q) * C + ch) = make_float4(vv[0], vv[1], vv[2], vv[3]);
                    } else {
                        Quad<E> hi, lo;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            hi.e[i] = (E)vv[i];
                            lo.e[i] = (E)(vv[i] - (float)hi.e[i]);
                        }
                        *reinterpret_cast<Quad<E>*>(lds + off) = hi;
                        *reinterpret_cast<Quad<E>*>(lds + PSTR + off) = lo;
                    }
                }
            }
        }
        __syncthreads();                                        // C: the result is in X
        if (!has_next) break;
        t += stride;
    }
}

// ---- kernel 2c / c8: the two-image residual block on the c8 arithmetic (192 filters; round 4) --------------------------------
// k_resblock_ip's roles, images and barriers (X | Y | 16 shared zero rows; six matrix waves + two copy waves; the second
// epilogue in place over X; the copy waves drain X to HBM and refill it at barrier C) with c8k::kloop<..., 192> -- 384-byte
// pixel rows [f16 x 192] / [lo8 x 192 | e4m3(x) x 192], swizzled inside aligned groups of eight chunks, three 64-channel
// blocks per tap -- and k_resblock_c8's arithmetic: accumulators start at bias (K loop 1) / bias + skip (K loop 2, read from
// X by the owning lane), the epilogues only apply ReLU and split.  2.0 instead of 3.0 MFMA-equivalents per product for the
// reference's deployed 10 x 192 topology (configs/distribute.py:84-87).  Bit-identical to two cz_conv3x3_c8 launches.
// XF / YF (round 6): the formats of the image the first convolution reads and of the intermediate image -- 0 = c8 (e4m3
// corrections), 1 = c6 (bf6 pieces with an exponent: cz_conv3x3_c6_pack_weights filters; 25 % less matrix time per product).
// <0, 0>: the c8 block; <1, 1>: a c6 block; <0, 1>: the tower's first c6 block, whose input is the input layer's c8 image.
// A c6 block's result is a c6 image with its second filter's output exponent -- or a c8 image where that filter carries
// y_exp = 127 (the hand-over of a c6>N tower), or fp32 (y_f32).  The c6 pieces are formed exactly as in k_resblock_c8<.., C6>
// (tiles trade lane halves with v_permlane32_swap, v_cvt_scalef32_2xpk16_bf6_f32); piece (kind, 32-channel block w) of a pixel
// row has its 16-byte head in chunk kind * CPR / 2 + 4 (w >> 1) + 2 (w & 1), its 8-byte tail at the start of the next chunk.
// CHAIN (round 6, cz_resblock_chain): ch.n consecutive blocks of ONE format per launch.  Two images leave no room for a second
// board, so a workgroup takes ONE board through all blocks: the in-place second epilogue already leaves block b's result in X
// as block b + 1's input, and the drain to HBM + refill (69 KB through two copy waves, all matrix waves waiting) happens once
// per chain instead of once per block.  Biases double-buffered in LDS by the running block count; filters and image exponents
// switch per block; y_f32 applies to the chain's last block.  Same arithmetic as ch.n one-block launches: bit-identical.
template <int C, int XF = 0, int YF = 0>
__global__ __launch_bounds__((C / 32) * 64 + ip::COPY_THREADS, 1) void k_resblock_ip_c8(
    const _Float16* __restrict__ xh, const unsigned char* __restrict__ xc, BlockChain<ip::MAX_BLOCKS> ch, _Float16* __restrict__ yh,
    unsigned char* __restrict__ yc, float* __restrict__ yf_last, int n_boards, const int32_t* __restrict__ n_dev)
{
    typedef Geom<C, 1, 2> G;
    constexpr int RB = G::RB, CPR = G::CPR, CT = G::CT, NT = 3;
    constexpr int PSTR = ip::ROWS * RB;                         // bytes per operand part
    constexpr int BIAS_OFF = 2 * PSTR;
    constexpr int CTHR = ip::COPY_THREADS, CHUNKS = 90 * CPR, LITER = (CHUNKS + CTHR - 1) / CTHR;
    __shared__ __attribute__((aligned(16))) unsigned char lds[BIAS_OFF + 2 * 2 * C * 4];       // bias[2 buffers][2 convolutions][C]
    const int NB = ch.n;
    static_assert(sizeof(lds) <= 160 * 1024, "two images + zero rows must fit the CU's LDS");
    n_boards = nn_live_boards(n_boards, n_dev);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int stride = gridDim.x;
    int t = blockIdx.x;
    if (t >= n_boards) return;
    auto chunk_off = [&](int i) {                               // chunk i of a board (row i / CPR, chunk i % CPR) in the X image
        const int row = i / CPR, ch = i - row * CPR;
        return row * RB + ((ch & ~G::SWZ) << 4) + (((ch ^ row) & G::SWZ) << 4);
    };

    if (wave >= CT) {                                           // ---- copy waves ----
        const int ctid = tid - CT * 64;
        uint4 v[2][LITER];
        auto fetch = [&](int board) {
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                const uint4* src = part ? reinterpret_cast<const uint4*>(xc + (size_t)board * 90 * 2 * C)
                                        : reinterpret_cast<const uint4*>(xh + (size_t)board * 90 * C);
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    const int i = it * CTHR + ctid;
                    v[part][it] = make_uint4(0, 0, 0, 0);
                    if ((it + 1) * CTHR <= CHUNKS || i < CHUNKS) v[part][it] = src[i];
                }
            }
        };
        auto put = [&]() {
#pragma unroll
            for (int part = 0; part < 2; ++part)
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    const int i = it * CTHR + ctid;
                    if ((it + 1) * CTHR <= CHUNKS || i < CHUNKS)
                        *reinterpret_cast<uint4*>(lds + part * PSTR + chunk_off(i)) = v[part][it];
                }
        };
        auto drain = [&](int board, bool refill) {
#pragma unroll
            for (int part = 0; part < 2; ++part) {
                uint4* dst = part ? reinterpret_cast<uint4*>(yc + (size_t)board * 90 * 2 * C)
                                  : reinterpret_cast<uint4*>(yh + (size_t)board * 90 * C);
#pragma unroll
                for (int it = 0; it < LITER; ++it) {
                    const int i = it * CTHR + ctid;
                    if (!((it + 1) * CTHR <= CHUNKS || i < CHUNKS)) continue;
                    unsigned char* a = lds + part * PSTR + chunk_off(i);
                    if (!yf_last) dst[i] = *reinterpret_cast<const uint4*>(a);
                    if (refill) *reinterpret_cast<uint4*>(a) = v[part][it];
                }
            }
        };
        fetch(t);
        put();
        for (int i = ctid; i < 16 * CPR; i += CTHR) {           // the shared zero rows, both parts
            *reinterpret_cast<uint4*>(lds + ip::ROW_Z * RB + i * 16) = make_uint4(0, 0, 0, 0);
            *reinterpret_cast<uint4*>(lds + PSTR + ip::ROW_Z * RB + i * 16) = make_uint4(0, 0, 0, 0);
        }
        // biases of running block g (block g % NB) into buffer g & 1
        auto write_bias = [&](int g) {
            const int blk = g % NB;
            float* dst = reinterpret_cast<float*>(lds + BIAS_OFF) + (g & 1) * 2 * C;
            for (int i = ctid; i < C; i += CTHR) {
                dst[i] = ch.b1[blk][i];
                dst[C + i] = ch.b2[blk][i];
            }
        };
        write_bias(0);
        write_bias(1);                                          // (one block per launch: both buffers hold its biases)
        int g = 0;
        for (;;) {
            __syncthreads();                                    // A: X holds board t
            const int tn = t + stride;
            const bool has_next = tn < n_boards;
            if (has_next) fetch(tn);
            for (int b = 0; b < NB; ++b, ++g) {
                __syncthreads();                                // B: Y complete; block g's biases are consumed
                if (NB > 1) write_bias(g + 2);                  // (one block per launch: its biases never change)
                __syncthreads();                                // C: the block's result is in X
            }
            drain(t, has_next);
            if (!has_next) break;
            t = tn;
        }
        return;
    }

    // ---- matrix waves ----
    const int kb = lane >> 5, ln = lane & 31;
    // byte offset (inside a part) of 16-byte chunk `chunk` of pixel row `row_abs`, swizzle key = the image-relative row
    auto choff = [&](int row_abs, int key, int chunk) {
        return row_abs * RB + ((chunk & ~G::SWZ) << 4) + (((chunk ^ key) & G::SWZ) << 4);
    };
    // relu'd fp32 accumulators of the three tiles -> the c6 operand triple of image `row0` (its first absolute row) with
    // exponent k: f16 quads per lane, the two bf6 pieces of a pixel's 32 channels after the lane halves traded tiles.
    // acc keeps relu(acc).
    auto write_c6 = [&](f32x16* acc, int row0, int k, int ln2, int kb2) __attribute__((always_inline)) {
        using rb8::u32x6;
        const float s_hi = __builtin_ldexpf(1.0f, k), s_lo = __builtin_ldexpf(1.0f, k - cf8::X_LO_SHIFT);
        f32x16 lo[NT];
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int q = p * 32 + ln2;
            const int row = q < 90 ? q : 89;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = wave * 32 + g * 8 + kb2 * 4;
                Quad<_Float16> hq;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float r = acc[p][g * 4 + i] > 0.0f ? acc[p][g * 4 + i] : 0.0f;
                    hq.e[i] = (_Float16)r;
                    acc[p][g * 4 + i] = r;
                    lo[p][g * 4 + i] = r - (float)hq.e[i];
                }
                if (q < 90) *reinterpret_cast<Quad<_Float16>*>(lds + choff(row0 + row, row, ch >> 3) + (ch & 7) * 2) = hq;
            }
        }
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {                       // pair (0, 1), then tile 2 with itself
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
                const int c0 = 4 * (wave >> 1) + 2 * (wave & 1), c1 = CPR / 2 + c0;
                unsigned char* P1 = lds + PSTR;
                *reinterpret_cast<uint4*>(P1 + choff(row0 + q, q, c0)) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
                *reinterpret_cast<uint2*>(P1 + choff(row0 + q, q, c0 + 1)) = make_uint2(pl[4], pl[5]);
                *reinterpret_cast<uint4*>(P1 + choff(row0 + q, q, c1)) = make_uint4(pv[0], pv[1], pv[2], pv[3]);
                *reinterpret_cast<uint2*>(P1 + choff(row0 + q, q, c1 + 1)) = make_uint2(pv[4], pv[5]);
            }
        }
    };
    // offsets of this lane's four channels ch .. ch + 3 of pixel row `row` (image-relative key for the swizzle): the f16 quad,
    // its lo8 word, its e4m3(x) word
    auto offs = [&](int row_abs, int key, int ch, int& off, int& off_lo, int& off_hi) {
        const int c_f = ch >> 3, c_lo = ch >> 4, c_hi = CPR / 2 + (ch >> 4);
        off = row_abs * RB + ((c_f & ~G::SWZ) << 4) + (((c_f ^ key) & G::SWZ) << 4) + (ch & 7) * 2;
        off_lo = PSTR + row_abs * RB + ((c_lo & ~G::SWZ) << 4) + (((c_lo ^ key) & G::SWZ) << 4) + (ch & 15);
        off_hi = PSTR + row_abs * RB + ((c_hi & ~G::SWZ) << 4) + (((c_hi ^ key) & G::SWZ) << 4) + (ch & 15);
    };
    int g = 0;                                                  // running block count: its parity picks the bias buffer
    for (;;) {
        __syncthreads();                                        // A
        const bool has_next = t + stride < n_boards;
      for (int blk = 0; blk < NB; ++blk, ++g) {
        const void* w1p = ch.w1[blk];
        const void* w2p = ch.w2[blk];
        const c8k::Filter flt1 = c8k::make_filter<C>(w1p, wave, lane), flt2 = c8k::make_filter<C>(w2p, wave, lane);
        const float* bias1 = reinterpret_cast<const float*>(lds + BIAS_OFF) + (g & 1) * 2 * C;
        const float* bias2 = bias1 + C;
        // c6: the exponents of the images the two convolutions read and of the one the block writes (127: a c8 image)
        const int* ints1 = reinterpret_cast<const int*>(reinterpret_cast<const uint4*>(w1p) + c8k::Geo<C>::MAIN_U4 + c8k::Geo<C>::C8_U4);
        const int* ints2 = reinterpret_cast<const int*>(reinterpret_cast<const uint4*>(w2p) + c8k::Geo<C>::MAIN_U4 + c8k::Geo<C>::C8_U4);
        const int k_x = XF ? __builtin_amdgcn_readfirstlane(ints1[2]) : 0;
        const int k_y = YF ? __builtin_amdgcn_readfirstlane(ints2[2]) : 0;
        const int k_out = YF ? __builtin_amdgcn_readfirstlane(ints2[3]) : CZ_C6_OUT_C8;
        float* yf = blk == NB - 1 ? yf_last : nullptr;          // fp32 output: the chain's last block only
        f32x16 acc[NT];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 bv = *reinterpret_cast<const float4*>(bias1 + wave * 32 + g * 8 + kb * 4);
#pragma unroll
            for (int p = 0; p < NT; ++p) {
                acc[p][g * 4 + 0] = bv.x; acc[p][g * 4 + 1] = bv.y; acc[p][g * 4 + 2] = bv.z; acc[p][g * 4 + 3] = bv.w;
            }
        }
        __builtin_amdgcn_s_setprio(3);
        c8k::kloop<NT, c8k::NoShadow, 0, false, C, XF>(lds, c8k::Image{0, ip::ROW_Z, PSTR}, flt1, lane, acc, 127 + k_x - cf8::X_LO_SHIFT, 127 + k_x);
        __builtin_amdgcn_s_setprio(0);
        int ln2 = ln, kb2 = kb;
        asm volatile("" : "+v"(ln2), "+v"(kb2));
        // epilogue 1: relu(acc) -> the operand triple (format YF) -> Y; the freed accumulators restart at b2 + skip (this lane's
        // own elements of X, format XF)
        if (YF) write_c6(acc, ip::ROW_Y, k_y, ln2, kb2);
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int q = p * 32 + ln2;
            const int row = q < 90 ? q : 89;
            rb8::f32x32 xl;
            if (XF) {                                           // this lane's elements of the x_lo piece of its 32-channel block
                const int c0 = 4 * (wave >> 1) + 2 * (wave & 1);
                const uint4 hd4 = *reinterpret_cast<const uint4*>(lds + PSTR + choff(row, row, c0));
                const uint2 tl2 = *reinterpret_cast<const uint2*>(lds + PSTR + choff(row, row, c0 + 1));
                const uint32_t wv[7] = {hd4.x, hd4.y, hd4.z, hd4.w, tl2.x, tl2.y, 0u};
                const uint32_t sh6 = (uint32_t)kb2 * 6u;       // (the upper lane half wants the odd elements: see k_resblock_c8)
                rb8::u32x6 pc;
#pragma unroll
                for (int w = 0; w < 6; ++w) pc[w] = __builtin_amdgcn_alignbit(wv[w + 1], wv[w], sh6);
                xl = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(pc, __builtin_ldexpf(1.0f, k_x - cf8::X_LO_SHIFT));
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = wave * 32 + g * 8 + kb2 * 4;
                int ox, oxl, oxh, oy, oyl, oyh;
                offs(row, row, ch, ox, oxl, oxh);
                offs(ip::ROW_Y + row, row, ch, oy, oyl, oyh);
                if (!YF) {
                    float r[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) r[i] = acc[p][g * 4 + i] > 0.0f ? acc[p][g * 4 + i] : 0.0f;
                    const cf8::Split4 o = cf8::split4(r);
                    if (q < 90) {
                        *reinterpret_cast<Quad<_Float16>*>(lds + oy) = o.hi;
                        *reinterpret_cast<uint32_t*>(lds + oyl) = o.l8;
                        *reinterpret_cast<uint32_t*>(lds + oyh) = o.h8;
                    }
                }
                const float4 bv = *reinterpret_cast<const float4*>(bias2 + ch);
                float vv[4] = {bv.x, bv.y, bv.z, bv.w};
                if (XF) {
                    const Quad<_Float16> xq = *reinterpret_cast<const Quad<_Float16>*>(lds + ox);
#pragma unroll
                    for (int i = 0; i < 4; ++i) vv[i] += (float)xq.e[i] + xl[2 * (g * 4 + i)];
                } else {
                    cf8::add_pair4(vv, *reinterpret_cast<const Quad<_Float16>*>(lds + ox), *reinterpret_cast<const uint32_t*>(lds + oxl));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[p][g * 4 + i] = vv[i];
            }
        }
        __syncthreads();                                        // B: Y complete
        __builtin_amdgcn_s_setprio(3);
        c8k::kloop<NT, c8k::NoShadow, 0, false, C, YF>(lds, c8k::Image{ip::ROW_Y, ip::ROW_Z, PSTR}, flt2, lane, acc,
                                                       127 + k_y - cf8::X_LO_SHIFT, 127 + k_y);
        __builtin_amdgcn_s_setprio(0);
        asm volatile("" : "+v"(ln2), "+v"(kb2));
        // epilogue 2: relu(acc) -> the operand triple in place over the skip operand (X is dead: every lane consumed its skip
        // elements before barrier B), or fp32 straight to HBM for the last block of a tower
        if (YF && !yf && k_out != CZ_C6_OUT_C8) write_c6(acc, 0, k_out, ln2, kb2);
        else
#pragma unroll
        for (int p = 0; p < NT; ++p) {
            const int q = p * 32 + ln2;
            if (q < 90) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int ch = wave * 32 + g * 8 + kb2 * 4;
                    float r[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) r[i] = acc[p][g * 4 + i] > 0.0f ? acc[p][g * 4 + i] : 0.0f;
                    if (yf) {
                        *reinterpret_cast<float4*>(yf + ((size_t)t * 90 + q) * C + ch) = make_float4(r[0], r[1], r[2], r[3]);
                    } else {
                        int ox, oxl, oxh;
                        offs(q, q, ch, ox, oxl, oxh);
                        const cf8::Split4 o = cf8::split4(r);
                        *reinterpret_cast<Quad<_Float16>*>(lds + ox) = o.hi;
                        *reinterpret_cast<uint32_t*>(lds + oxl) = o.l8;
                        *reinterpret_cast<uint32_t*>(lds + oxh) = o.h8;
                    }
                }
            }
        }
        __syncthreads();                                        // C: the result is in X
      }
        if (!has_next) break;
        t += stride;
    }
}

}  // namespace
