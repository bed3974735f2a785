// xq_conv_single.h -- part of xq_conv.hip's translation unit; do not compile it into a second one: the unit's device code is
// compared kernel by kernel when text moves between these headers (EXPERIMENTS.md, "the convolution unit's text in headers"), and
// the search unit's kernels changed by 0.4-1.7 % when part of that unit was compiled alone.
//
// One convolution per launch: k_conv3x3 (kernel 1) and its c8 form k_conv3x3_c8, with the c8 arithmetic's description.
#pragma once
#include "xq_c8_kloop.h"
#include "xq_conv_kloop.h"

namespace {

// ---- kernel 1: one workgroup = P boards, one pass (any channel count; used for the small / plain-precision cases) --
template <typename E, int C, int P, int PARTS, int MINW>
__global__ __launch_bounds__(C / 32 * 64, MINW) void k_conv3x3(
    const E* __restrict__ xh, const E* __restrict__ xl, const E* __restrict__ wp, const float* __restrict__ bias,
    const E* __restrict__ sh, const E* __restrict__ sl, E* __restrict__ yh, E* __restrict__ yl,
    float* __restrict__ yf, int n_boards, int relu)
{
    typedef Geom<C, P, PARTS> G;
    constexpr int NT = G::NT;
    __shared__ __attribute__((aligned(16))) unsigned char lds[G::REGION];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * P;
    {
        uint4 v[PARTS][G::ITER];
        tile_load<E, C, P, PARTS>(xh, xl, n0, n_boards, tid, v);
        tile_write<C, P, PARTS>(lds, tid, v);
        zero_rows_write<C, P, PARTS>(lds, tid);
    }
    __syncthreads();

    f32x16 acc[NT];
    conv_kloop<E, C, P, PARTS>(lds, reinterpret_cast<const uint4*>(wp) + wave * 64 + lane, lane, acc);

    // ---- epilogue: lane holds, for pixel (tile p, column ln), channels 32*wave + 8*g + 4*kb + {0..3}, g = 0..3 ----
    const int kb = lane >> 5, ln = lane & 31;
    // everything the epilogue reads from memory is requested up front (round 6: with a load next to every store the compiler
    // waited for each -- 4 NT bias + skip round trips in a row; a one-board batch, the `mini` configuration, felt every one)
    f32x4 bq[4];
    c8k::u32x2 skh[NT][4], skl[NT][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bq[g] = *reinterpret_cast<const f32x4*>(bias + wave * 32 + g * 8 + kb * 4);
#pragma unroll
    for (int p = 0; p < NT; ++p) {
        const int q = (p % 3) * 32 + ln;
        const int n = n0 + p / 3;
        const bool live = q < 90 && n < n_boards;
        const size_t pix = ((size_t)(live ? n : 0) * 90 + (live ? q : 0)) * C;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = wave * 32 + g * 8 + kb * 4;
            skh[p][g] = c8k::u32x2{0u, 0u};
            skl[p][g] = c8k::u32x2{0u, 0u};
            if (sh && live) {
                skh[p][g] = *reinterpret_cast<const c8k::u32x2*>(sh + pix + ch);
                if (PARTS == 2) skl[p][g] = *reinterpret_cast<const c8k::u32x2*>(sl + pix + ch);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(bq[g]));
#pragma unroll
    for (int p = 0; p < NT; ++p) {
        const int q = (p % 3) * 32 + ln;
        const int n = n0 + p / 3;
        if (q >= 90 || n >= n_boards) continue;
        const size_t pix = ((size_t)n * 90 + q) * C;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = wave * 32 + g * 8 + kb * 4;
            const f32x4 bv = bq[g];
            float v[4] = {acc[p][g * 4 + 0] + bv[0], acc[p][g * 4 + 1] + bv[1], acc[p][g * 4 + 2] + bv[2],
                          acc[p][g * 4 + 3] + bv[3]};
            if (sh) {
                const Quad<E> a = __builtin_bit_cast(Quad<E>, skh[p][g]);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += (float)a.e[i];
                if (PARTS == 2) {
                    const Quad<E> b2 = __builtin_bit_cast(Quad<E>, skl[p][g]);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += (float)b2.e[i];
                }
            }
            if (relu) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.0f ? v[i] : 0.0f;
            }
            if (yf) {
                *reinterpret_cast<float4*>(yf + pix + ch) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                Quad<E> hi, lo;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    hi.e[i] = (E)v[i];
                    lo.e[i] = (E)(v[i] - (float)hi.e[i]);
                }
                *reinterpret_cast<Quad<E>*>(yh + pix + ch) = hi;
                if (PARTS == 2) *reinterpret_cast<Quad<E>*>(yl + pix + ch) = lo;
            }
        }
    }
}

// ---- the c8 tower arithmetic: fp16 main term + two block-scaled fp8 correction terms --------------------------------
// The tower is bound by the socket's power cap and spends three bf16 MFMAs per product.  With an fp16 main
// term (11 bits) the correction terms  w_hi x_lo  and  w_lo x_hi  need four significant bits, which is what an e4m3 operand
// holds:   w x  ~  f16(w) f16(x)  +  e4m3(w) e4m3(x - f16(x))  +  e4m3(w - f16(w)) e4m3(x)
// as v_mfma_f32_32x32x16_f16 + 2 x v_mfma_scale_f32_32x32x64_f8f6f4 per 64 input channels: 2.0 instead of 3.0 MFMA-equivalents
// per product (measured 1.47x in register-resident loops, profiles/r03_fp8_corrections_study.json; per-product accuracy
// 2^-16, policy within 2e-5 of float64 in the emulated 7 x 128 network, same file).  k_conv3x3_c8 is the single-convolution
// form (cz_conv3x3_c8); k_resblock<..., C8> (dtype CZ_F16C8) is the residual block the self-play engine runs by default,
// k_input_conv<..., C8> produces its operands; the pipelined block (k_resblock_pipe) still computes the bf16 arithmetic.
//   operands: x_hi f16 [n][90][C];  x_c8 bytes [n][90][2C] = e4m3(x_lo * 2^11) for the C channels, then e4m3(x) for them
//   LDS:      part 0 = x_hi rows, part 1 = x_c8 rows (same 2C bytes per pixel: the image code of the split kernels serves)
//   weights:  f16 fragments as in cz_conv3x3_pack_weights, then per (tap, 64-channel block, kind) two 16-byte pieces per
//             lane: kind 0 = e4m3(w * 2^sh) (meets x_lo), kind 1 = e4m3((w - f16(w)) * 2^sl) (meets e4m3(x)); lane l holds
//             output channel l % 32, input channels 32 (l / 32) .. + 31 of the block -- the same k map as the pixels;
//             the power-of-two scales sh, sl follow the fragments
template <int C, int P>
__global__ __launch_bounds__(C / 32 * 64, 1) void k_conv3x3_c8(
    const _Float16* __restrict__ xh, const unsigned char* __restrict__ xc, const uint4* __restrict__ wp,
    const float* __restrict__ bias, const _Float16* __restrict__ sh, const unsigned char* __restrict__ sc8,
    _Float16* __restrict__ yh, unsigned char* __restrict__ yc, float* __restrict__ yf, int n_boards, int relu)
{
    typedef Geom<C, P, 2> G;
    constexpr int NT = G::NT;
    __shared__ __attribute__((aligned(16))) unsigned char lds[G::REGION];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * P;
    {
        uint4 v[2][G::ITER];
        tile_load<_Float16, C, P, 2>(xh, reinterpret_cast<const _Float16*>(xc), n0, n_boards, tid, v);
        tile_write<C, P, 2>(lds, tid, v);
        zero_rows_write<C, P, 2>(lds, tid);
    }
    __syncthreads();
    static_assert(cf8::Pack<C>::MAIN_U4 == c8k::Geo<C>::MAIN_U4 && cf8::Pack<C>::C8_U4 == c8k::Geo<C>::C8_U4, "packed layout");
    // The accumulators start at bias (+ the skip operand, hi + lo8 * 2^-11): the products are added on top and the epilogue
    // has only the ReLU and the split left.  Same order in k_resblock_c8, so the two stay bit-identical.
    const int kb = lane >> 5, ln = lane & 31;
    f32x16 acc[NT];
#pragma unroll
    for (int p = 0; p < NT; ++p) {
        const int q = (p % 3) * 32 + ln;
        const int n = n0 + p / 3;
        const bool live = q < 90 && n < n_boards;
        const size_t pixel = (size_t)(live ? n : 0) * 90 + (live ? q : 0);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = wave * 32 + g * 8 + kb * 4;
            const float4 bv = *reinterpret_cast<const float4*>(bias + ch);
            float v[4] = {bv.x, bv.y, bv.z, bv.w};
            if (sh && live)
                cf8::add_pair4(v, *reinterpret_cast<const Quad<_Float16>*>(sh + pixel * C + ch),
                              *reinterpret_cast<const uint32_t*>(sc8 + pixel * 2 * C + ch));
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[p][g * 4 + i] = v[i];
        }
    }
    c8k::kloop<NT, c8k::NoShadow, 0, false, C>(lds, c8k::Image{0, G::ZROW, G::PART_BYTES}, c8k::make_filter<C>(wp, wave, lane),
                                               lane, acc, 127 - cf8::X_LO_SHIFT, 127);
#pragma unroll
    for (int p = 0; p < NT; ++p) {
        const int q = (p % 3) * 32 + ln;
        const int n = n0 + p / 3;
        if (q >= 90 || n >= n_boards) continue;
        const size_t pixel = (size_t)n * 90 + q;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int ch = wave * 32 + g * 8 + kb * 4;
            float v[4] = {acc[p][g * 4 + 0], acc[p][g * 4 + 1], acc[p][g * 4 + 2], acc[p][g * 4 + 3]};
            if (relu) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = v[i] > 0.0f ? v[i] : 0.0f;
            }
            if (yf) {
                *reinterpret_cast<float4*>(yf + pixel * C + ch) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                const cf8::Split4 o = cf8::split4(v);
                *reinterpret_cast<Quad<_Float16>*>(yh + pixel * C + ch) = o.hi;
                *reinterpret_cast<uint32_t*>(yc + pixel * 2 * C + ch) = o.l8;
                *reinterpret_cast<uint32_t*>(yc + pixel * 2 * C + C + ch) = o.h8;
            }
        }
    }
}

}  // namespace
