// xq_conv.hip -- the convolutions of the policy/value ResNet as hand-written MFMA kernels (gfx950).
//
//   conv_kloop      the shared K loop (9 taps x C channels out of an LDS image, weights streamed from L2)
//   k_conv3x3       kernel 1: one convolution per launch, P boards per workgroup (any supported filter count / mode)
//   k_resblock      kernel 2: a whole residual block per launch, persistent, matrix waves + copy waves; optionally the
//                   two 1x1 head convolutions folded into the last block's store pass
//   k_input_conv    kernel 3: the 5x5 input convolution on the feature planes as the search kernel writes them
//   k_split_bias_act  fp32 -> operand pair (used when the input layer comes from a library convolution)
//
// Reference: the residual tower of CChessModel.build / _build_residual_block (cchess_alphazero/agent/model.py:40-83):
// Conv2D(F, 3, padding="same", use_bias=False) -> BatchNorm -> (+ skip) -> ReLU on 10x9 boards.  With BatchNorm folded
// into the weights this is  y = act(conv3x3(x, w) + bias (+ skip))  and it is 97 % of the FLOPs of a self-play round.
//
// Design (not an im2col GEMM, not a library call):
//   * one workgroup = P whole boards.  Their activations ([90 pixels][C] channels-last, 2-byte elements) are copied
//     ONCE into LDS; all 9 taps x C input channels are then read from that LDS image, so HBM/L2 sees every
//     activation exactly once per layer.  Pixel rows are XOR-swizzled by (row & 15) in 16-byte chunks so that the
//     32 rows a ds_read_b128 touches fall on 16 distinct bank slots per lane group; out-of-board taps point at an
//     all-zero row instead of being predicated.
//   * wave w owns output channels [32w, 32w+32) for every pixel of the P boards: v_mfma_f32_32x32x16 with the
//     WEIGHTS as the A operand (rows = output channels) and the PIXELS as the B operand (columns = pixels), so each
//     lane ends up with 4 runs of 4 consecutive channels of one pixel -> 8-byte channels-last stores.
//     The weights are pre-packed on the host in exactly fragment order (cz_conv3x3_pack_weights): every weight load
//     is one fully coalesced 1 KiB global_load_dwordx4 per wave, served from L2 (the whole packed filter is < 1.2 MiB),
//     prefetched three K-steps ahead through a 4-deep register ring.  The K loop has no barrier at all.
//   * precision.  parts = 1: operands are bf16 (or fp16), fp32 accumulate.  parts = 2 ("split" mode): every operand is
//     a (hi, lo) pair of bf16 with hi + lo equal to the fp32 value to 2^-17, and the kernel accumulates
//     hi*hi + hi*lo + lo*hi in fp32 -- three bf16 MFMAs (1/16 the cost of an fp32 MFMA each) give a product error of
//     ~1e-5 relative, which keeps policy/value within the 1e-4 the parity contract asks for while running at several
//     times the fp32 matrix rate.  The epilogue re-splits its fp32 result into (hi, lo) for the next layer.
//     E = _Float16 ("f16x3"): (hi, lo) fp16 pairs, the same three MFMAs; a pair holds v to 2^-22 |v| + 2^-25 because the
//     matrix unit honours fp16 subnormals (a filter tap's lo part usually is one).  Every kernel on these pairs is held to
//     a float64 model of exactly this arithmetic, element by element: tests/test_gpu_f16x3.py, bounds in tests/f16_pairs.py.
//     Plain operands and bf16 pairs are held to the same model (one term per K-step, the bf16 pair format) in
//     tests/test_gpu_plain_bf16x3.py: cz_conv3x3 and cz_input_conv per element, their 2-byte stores bit for bit.
//   * epilogue fused: + bias, + skip (read as hi + lo), ReLU, split / convert, store.  The last trunk layer can
//     emit fp32 directly (y_f32) for the policy/value heads.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include <math.h>
#include "../../include/czero.h"
#include "xq_c8_kloop.h"
#include "xq_nn_common.h"
#include "xq_nn_launch.h"
#include "xq_conv_geom.h"       // Geom, the in-place chains' rows (shared with csrc/xq_conv_ip4.hip)
#include "xq_conv_ip4.h"        // k_resblock_ip4_c8 and its launch: the 192-filter instantiations are this unit's

namespace {

// global -> registers: the P boards starting at board n0 (16 bytes per lane per iteration, fully coalesced)
template <typename E, int C, int P, int PARTS, int NTHR = Geom<C, P, PARTS>::GTHREADS>
__device__ __forceinline__ void tile_load(const E* xh, const E* xl, int n0, int n_boards, int gtid,
                                          uint4 (*v)[(Geom<C, P, PARTS>::CHUNKS + NTHR - 1) / NTHR])
{
    typedef Geom<C, P, PARTS> G;
    constexpr int ITER = (G::CHUNKS + NTHR - 1) / NTHR;
    const bool full = n0 + P <= n_boards;
#pragma unroll
    for (int part = 0; part < PARTS; ++part) {
        const uint4* src = reinterpret_cast<const uint4*>((part ? xl : xh) + (size_t)n0 * 90 * C);
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int i = it * NTHR + gtid;
            const bool ok = ((it + 1) * NTHR <= G::CHUNKS || i < G::CHUNKS) &&
                            (full || n0 + i / (G::CPR * 90) < n_boards);
            v[part][it] = make_uint4(0, 0, 0, 0);
            if (ok) v[part][it] = src[i];
        }
    }
}

// registers -> LDS image: [row][chunk ^ (row & SWZ)], plus the all-zero row
template <int C, int P, int PARTS, int NTHR = Geom<C, P, PARTS>::GTHREADS>
__device__ __forceinline__ void tile_write(unsigned char* region, int gtid,
                                           const uint4 (*v)[(Geom<C, P, PARTS>::CHUNKS + NTHR - 1) / NTHR])
{
    typedef Geom<C, P, PARTS> G;
    constexpr int ITER = (G::CHUNKS + NTHR - 1) / NTHR;
#pragma unroll
    for (int part = 0; part < PARTS; ++part) {
        unsigned char* dst = region + part * G::PART_BYTES;
#pragma unroll
        for (int it = 0; it < ITER; ++it) {
            const int i = it * NTHR + gtid;
            const int row = i / G::CPR, ch = i % G::CPR;
            if ((it + 1) * NTHR <= G::CHUNKS || i < G::CHUNKS)
                *reinterpret_cast<uint4*>(dst + row * G::RB + ((ch ^ (row & G::SWZ)) << 4)) = v[part][it];
        }
    }
}

// the 16 all-zero rows of an image (written once per workgroup: nothing else ever stores there)
template <int C, int P, int PARTS, int NTHR = Geom<C, P, PARTS>::GTHREADS>
__device__ __forceinline__ void zero_rows_write(unsigned char* region, int gtid)
{
    typedef Geom<C, P, PARTS> G;
#pragma unroll
    for (int part = 0; part < PARTS; ++part)
        for (int i = gtid; i < G::ZROWS * G::CPR; i += NTHR)
            *reinterpret_cast<uint4*>(region + part * G::PART_BYTES + G::ZROW * G::RB + i * 16) = make_uint4(0, 0, 0, 0);
}

// The K loop: 9 taps x C input channels for the 32 output channels of this wave and all NT pixel tiles of the
// LDS image.  acc[p][r] <-> pixel (p % 3) * 32 + (lane & 31) of board p / 3,
//                          channel 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
//   row_base / zrow / part_bytes: where the image's first row, the 16 zero rows and the second operand part are, for
//   kernels whose images share one LDS allocation (k_resblock_ip); the defaults are the self-contained layout of Geom.
//   CTW: channel tiles per wave (wq points at the wave's FIRST tile; the tiles of a K-step are 64 uint4 apart).  Every
//   pixel fragment read from LDS then feeds CTW MFMAs: with plain operands and one tile per wave there is one
//   ds_read_b128 (8 LDS cycles) per MFMA (32 cycles of one of four SIMDs), i.e. the LDS port is as busy as the matrix
//   pipes; two tiles per wave halve that.  acc[c * NT + p] <-> channel tile c of the wave.
template <typename E, int C, int P, int PARTS, int CTW = 1>
__device__ __forceinline__ void conv_kloop(const unsigned char* region, const uint4* wq, int lane,
                                           f32x16* acc, int row_base = 0, int zrow = Geom<C, P, PARTS>::ZROW,
                                           int part_bytes = Geom<C, P, PARTS>::PART_BYTES)
{
    typedef Geom<C, P, PARTS> G;
    typedef typename Mfma<E>::V8 V8;
    constexpr int NT = G::NT, KK = G::KK, W_RING = G::W_RING;
    static_assert(CTW == 1 || PARTS == 1, "several channel tiles per wave: plain operands only");
    const int kb = lane >> 5, ln = lane & 31;
    // byte offset (within a part) of this lane's 16-byte fragment piece for K-step 0 of a tap: row*RB + swizzle bits.
    // chunk = 2*kk + kb, swizzled chunk = chunk ^ (row & SWZ) = (2*kk) ^ (kb ^ (row & SWZ)): the lane part is folded
    // into pre[], the K-step part is one XOR with the constant kk << 5.
    int pre[NT], pre_n[NT];
    int qy[3], qx[3];                                  // board row / column of this lane's pixel in each of the 3 tiles
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int q = t * 32 + ln;
        qy[t] = q < 90 ? q / 9 : 100;                  // 100: never on the board, whatever the tap
        qx[t] = q - (q / 9) * 9;
    }
    auto tap_row = [&](int dy, int dx, int p) {
        const int t = p % 3;
        const bool ok = (unsigned)(qy[t] + dy) < 10u && (unsigned)(qx[t] + dx) < 9u;
        const int nominal = (p / 3) * 90 + t * 32 + ln + dy * 9 + dx;
        const int row = ok ? row_base + nominal : zrow + (nominal & 15);
        // (swizzle key = the image-relative row; zrow is a multiple of 16, so a zero row keys like the row it stands for)
        return row * G::RB + (((kb ^ nominal) & G::SWZ) << 4);
    };
    constexpr int WP = PARTS * CTW;                    // weight fragments per K-step: [part] (CTW == 1) or [tile]
    V8 wf[W_RING][WP];
    V8 px[2][NT][PARTS];
#pragma unroll
    for (int p = 0; p < CTW * NT; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][r] = 0.0f;

    auto load_w = [&](int step, int f) {               // f: part (CTW == 1) or channel tile of the wave
        const int part = CTW == 1 ? f : 0, c = CTW == 1 ? 0 : f;
        return __builtin_bit_cast(V8, wq[(size_t)part * G::W_PART + (size_t)step * G::W_STEP + c * 64]);
    };
    auto load_px = [&](int off, int part) {
        return __builtin_bit_cast(V8, *reinterpret_cast<const uint4*>(region + part * part_bytes + off));
    };

#pragma unroll
    for (int p = 0; p < NT; ++p) pre[p] = tap_row(-1, -1, p);
#pragma unroll
    for (int s = 0; s < W_RING - 1; ++s)
#pragma unroll
        for (int f = 0; f < WP; ++f) wf[s][f] = load_w(s, f);
#pragma unroll
    for (int part = 0; part < PARTS; ++part)
#pragma unroll
        for (int p = 0; p < NT; ++p) px[0][p][part] = load_px(pre[p], part);

    // One K-step = NT (x3 in split mode) MFMAs.  The LDS reads of the NEXT K-step and the weight loads three K-steps
    // ahead are issued one per MFMA, in the shadow of the matrix pipe; sched_barrier pins that order (left alone, the
    // compiler sinks every load to just before its use and the pipe drains at each K-step).
    constexpr int NM = CTW * NT * (PARTS == 2 ? 3 : 1);
    constexpr int NL = NT * PARTS;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        // rows of the NEXT tap: computed a few at a time in the shadow of this tap's MFMAs (done in one block at the
        // tap boundary they leave the matrix pipe idle for ~400 cycles per tap)
        const int tn = tap < 8 ? tap + 1 : 8;
        const int ndy = tn / 3 - 1, ndx = tn - (tn / 3) * 3 - 1;
        constexpr int PER = (NT + KK - 2) / (KK - 1);    // rows to prepare per K-step: all done before the last step
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) {
            const int step = tap * KK + kk;
            const V8* w = wf[kk % W_RING];
            V8 (*b)[PARTS] = px[kk & 1];
            V8 (*bn)[PARTS] = px[(kk + 1) & 1];
            const int* rows = kk + 1 < KK ? pre : pre_n;
            const int kn = (kk + 1) % KK;
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                const int pass = i / NT, p = i % NT;      // pass 0: w_hi*x_hi, 1: w_lo*x_hi, 2: w_hi*x_lo
                if (CTW == 1) acc[p] = Mfma<E>::mma(w[pass == 1 ? PARTS - 1 : 0], b[p][pass == 2 ? PARTS - 1 : 0], acc[p]);
                else acc[i] = Mfma<E>::mma(w[pass], b[p][0], acc[i]);      // pass = channel tile of the wave
                if (i < NL) bn[i % NT][i / NT] = load_px(G::kstep(rows[i % NT], kn), i / NT);
                if (i >= NM - PER && kk * PER + (i - (NM - PER)) < NT)
                    pre_n[kk * PER + (i - (NM - PER))] = tap_row(ndy, ndx, kk * PER + (i - (NM - PER)));
                if (i >= NM - WP)
                    wf[(kk + W_RING - 1) % W_RING][i - (NM - WP)] = load_w(step + W_RING - 1, i - (NM - WP));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
#pragma unroll
        for (int p = 0; p < NT; ++p) pre[p] = pre_n[p];
    }
}

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
    if (n_dev) {                                        // compact queue: the board count lives on the device
        const int nd = __builtin_amdgcn_readfirstlane(*n_dev);
        n_boards = nd < n_boards ? nd : n_boards;
    }
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
    if (n_dev) {
        const int nd = __builtin_amdgcn_readfirstlane(*n_dev);
        n_boards = nd < n_boards ? nd : n_boards;
    }
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
// over the occupied squares (see k_resblock_pipe<FIRST> below: the same algorithm, here producing the c8 triple) instead
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
    if (n_dev) {                                        // compact queue: the board count lives on the device
        const int nd = __builtin_amdgcn_readfirstlane(*n_dev);
        n_boards = nd < n_boards ? nd : n_boards;
    }
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
        // ---- FIRST: the input layer of a board into v[][], in two halves (k_resblock_pipe<FIRST> documents the algorithm)
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
                pw[1] = lane < 32 ? fa.masks[slot * 96 + 64 + lane] : 0u;
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
                if (lane < 32) mk[64 + lane] = pw[1];
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

// (kernel 2d, the chain of 128-filter pair blocks in one launch -- k_tower_pairs4 -- lives in csrc/xq_tower.hip)

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
    if (n_dev) {
        const int nd = __builtin_amdgcn_readfirstlane(*n_dev);
        n_boards = nd < n_boards ? nd : n_boards;
    }
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
                pw[1] = lane < 32 ? fa.masks[slot * 96 + 64 + lane] : 0u;
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
                if (lane < 32) mk[64 + lane] = pw[1];
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
    if (n_dev) {
        const int nd = __builtin_amdgcn_readfirstlane(*n_dev);
        n_boards = nd < n_boards ? nd : n_boards;
    }
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
    if (n_dev) {
        const int nd = __builtin_amdgcn_readfirstlane(*n_dev);
        n_boards = nd < n_boards ? nd : n_boards;
    }
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

// ---- kernel 3: the input convolution (5x5, 14 or 28 feature planes -> C channels) ----------------------------------
// Reference: Conv2D(F, 5, padding="same") -> BatchNorm -> ReLU on the state_to_planes input (agent/model.py:36-39).
// The planes arrive exactly as the search kernel writes them ([in_planes][10][9] per board, values 0 / 1, any of
// fp32 / fp16 / bf16 / u8) and are transposed into a channels-last LDS image ([pixel][16 or 32 channels], zero padded)
// while being staged.  0 / 1 are exact in bf16, so only the WEIGHTS are split: two MFMAs per product in split mode.
// One K-step per tap and 16 input channels; output written as the (hi, lo) operand pair of the residual tower.
template <typename PT> __device__ __forceinline__ float plane_to_f(PT v) { return (float)v; }

template <typename E, typename PT, int C, int IC16, int P, int PARTS, bool C8 = false>
__global__ __launch_bounds__(C / 32 * 64, 1) void k_input_conv(
    const PT* __restrict__ planes, const E* __restrict__ wp, const float* __restrict__ bias, E* __restrict__ yh,
    E* __restrict__ yl, int n_boards, int in_planes, int relu, const int32_t* __restrict__ rows,
    const int32_t* __restrict__ n_dev)
{
    if (n_dev) {                                    // compact queue: the board count lives on the device
        const int nd = __builtin_amdgcn_readfirstlane(*n_dev);
        n_boards = nd < n_boards ? nd : n_boards;
        if ((int)blockIdx.x * P >= n_boards) return;
    }
    typedef typename Mfma<E>::V8 V8;
    constexpr int RBI = IC16 * 32;                  // bytes per pixel row of the input image
    // 16 zero rows and a swizzle, as in Geom: the 256-byte bank row holds RPB = 8 (or 4) of these short pixel rows, so
    // the 16 consecutive rows of a ds_read_b128 lane group would share 8 (4) slots; chunk ^= (row / RPB) gives each
    // of them its own 16-byte slot (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE was 0.60 here in round 1)
    constexpr int CPRI = IC16 * 2, RPB = 16 / CPRI;
    constexpr int ZROW = (P * 90 + 15) / 16 * 16;
    constexpr int IMG = (ZROW + 16) * RBI;
    constexpr int NT = P * 3, CT = C / 32, NTHR = CT * 64;
    constexpr int NX = NT * IC16;                   // operand reads per tap
    constexpr int NM = NX * PARTS;                  // MFMAs per tap
    constexpr int W_STEP = CT * 64;                 // uint4 per (tap, 16-channel group)
    constexpr int W_PART = (25 + 3) * IC16 * W_STEP;
    __shared__ __attribute__((aligned(16))) unsigned char img[IMG];
    __shared__ __attribute__((aligned(16))) unsigned char stage[PARTS * 90 * C * 2];    // one board of output

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * P;
    for (int i = tid; i < IMG / 16; i += NTHR) reinterpret_cast<uint4*>(img)[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    {
        const int per_board = in_planes * 90;
        const int nb = n_boards - n0 < P ? n_boards - n0 : P;
        // the image is all zero: only the occupied squares are written (a position has at most 32 of 1260 planes' bits set)
        auto put = [&](int bb, int c, int pix, float v) {
            const int row = bb * 90 + pix;
            *reinterpret_cast<E*>(img + row * RBI + (((c >> 3) ^ ((row / RPB) & (CPRI - 1))) << 4) + (c & 7) * 2) = (E)v;
        };
        if (sizeof(PT) == 1 && (per_board & 3) == 0) {
            // byte planes (what the search kernel writes for this network): four squares per load
            const int wpb = per_board >> 2;
            for (int i = tid; i < nb * wpb; i += NTHR) {
                const int bb = i / wpb, w = i - bb * wpb;
                // (compact queue: board n0 + bb of the batch is queue slot rows[n0 + bb])
                const uint32_t word = reinterpret_cast<const uint32_t*>(
                    reinterpret_cast<const unsigned char*>(planes) + (size_t)(rows ? rows[n0 + bb] : n0 + bb) * per_board)[w];
                if (word == 0u) continue;
                int c = (w * 4) / 90, pix = w * 4 - c * 90;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned b = (word >> (8 * k)) & 0xFFu;
                    if (b) put(bb, c, pix, (float)b);
                    if (++pix == 90) { pix = 0; ++c; }
                }
            }
        } else {
            for (int i = tid; i < nb * per_board; i += NTHR) {
                const int bb = i / per_board, r = i - bb * per_board;
                const PT* src = planes + (size_t)(rows ? rows[n0 + bb] : n0 + bb) * per_board - (size_t)bb * per_board;
                const int c = r / 90, pix = r - c * 90;
                const float v = plane_to_f(src[i]);
                if (v != 0.0f) put(bb, c, pix, v);
            }
        }
    }
    __syncthreads();

    const int kb = lane >> 5, ln = lane & 31;
    int qy[3], qx[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int q = t * 32 + ln;
        qy[t] = q < 90 ? q / 9 : 100;
        qx[t] = q - (q / 9) * 9;
    }
    auto tap_off = [&](int tap, int p, int g) {     // byte offset of this lane's 16 bytes for (tap, 16-channel group g)
        const int ky = tap / 5;
        const int dy = ky - 2, dx = tap - ky * 5 - 2;
        const int t = p % 3;
        const bool ok = (unsigned)(qy[t] + dy) < 10u && (unsigned)(qx[t] + dx) < 9u;
        const int nominal = (p / 3) * 90 + t * 32 + ln + dy * 9 + dx;
        const int row = ok ? nominal : ZROW + (nominal & 15);
        return row * RBI + ((((g << 1) | kb) ^ ((row / RPB) & (CPRI - 1))) << 4);
    };
    const uint4* wq = reinterpret_cast<const uint4*>(wp) + wave * 64 + lane;
    auto load_w = [&](int tap, int g, int part) {
        return __builtin_bit_cast(V8, wq[(size_t)part * W_PART + (size_t)(tap * IC16 + g) * W_STEP]);
    };
    V8 wf[4][IC16][PARTS];
    V8 px[2][NX];
    f32x16 acc[NT];
#pragma unroll
    for (int p = 0; p < NT; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][r] = 0.0f;
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int g = 0; g < IC16; ++g)
#pragma unroll
            for (int part = 0; part < PARTS; ++part) wf[s][g][part] = load_w(s, g, part);
#pragma unroll
    for (int i = 0; i < NX; ++i)
        px[0][i] = __builtin_bit_cast(V8, *reinterpret_cast<const uint4*>(img + tap_off(0, i % NT, i / NT)));

    auto tap_body = [&](int tap, const int ring, const int buf) {
        const int tn = tap < 24 ? tap + 1 : 24;
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int xi = i % NX, part = i / NX;          // all operands with w_hi first, then with w_lo
            acc[xi % NT] = Mfma<E>::mma(wf[ring][xi / NT][part], px[buf][xi], acc[xi % NT]);
            if (i < NX)
                px[buf ^ 1][i] = __builtin_bit_cast(
                    V8, *reinterpret_cast<const uint4*>(img + tap_off(tn, i % NT, i / NT)));
            if (i >= NM - IC16 * PARTS) {
                const int j = i - (NM - IC16 * PARTS);
                wf[(ring + 3) & 3][j / PARTS][j % PARTS] = load_w(tap + 3, j / PARTS, j % PARTS);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
#pragma unroll 1
    for (int t4 = 0; t4 < 24; t4 += 4) {
        tap_body(t4 + 0, 0, 0);
        tap_body(t4 + 1, 1, 1);
        tap_body(t4 + 2, 2, 0);
        tap_body(t4 + 3, 3, 1);
    }
    tap_body(24, 0, 0);

    // ---- epilogue: + bias, ReLU, split; one board at a time through an LDS staging image so that HBM sees whole
    // pixel rows (16 bytes per lane, 1 KiB per wave instruction).  Round 2 stored the accumulators straight from the
    // MFMA layout -- 8 bytes per lane, 32 different 256-byte rows per instruction -- and the layer ran at 1.5 TB/s:
    // 94 M sixteen-byte write requests per launch are a request-rate limit, not a bandwidth one.
    typedef Geom<C, 1, PARTS> GS;                   // staging geometry: [90 pixels][C] per part, chunks swizzled by row
    constexpr int SROWB = C * 2, SPART = 90 * SROWB;
    f32x4 bq[4];                                    // this wave's biases, fetched once (not once per 8-byte store: see k_resblock)
#pragma unroll
    for (int g = 0; g < 4; ++g) bq[g] = *reinterpret_cast<const f32x4*>(bias + wave * 32 + g * 8 + kb * 4);
#pragma unroll
    for (int g = 0; g < 4; ++g) asm volatile("" : "+v"(bq[g]));
#pragma unroll
    for (int bb = 0; bb < P; ++bb) {
        if (bb > 0) __syncthreads();                // the previous board has left the staging image
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int p = bb * 3 + t;
            const int q = t * 32 + ln;
            if (q >= 90) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int ch = wave * 32 + g * 8 + kb * 4;
                const f32x4 bv = bq[g];
                float v[4] = {acc[p][g * 4 + 0] + bv[0], acc[p][g * 4 + 1] + bv[1], acc[p][g * 4 + 2] + bv[2],
                              acc[p][g * 4 + 3] + bv[3]};
                const int off = q * SROWB + (((ch >> 3) ^ (q & GS::SWZ)) << 4) + (ch & 7) * 2;
                if constexpr (C8) {                 // the operand pair of the c8 arithmetic (k_conv3x3_c8): f16 row, then the c8 row
                    static_assert(!C8 || (PARTS == 2 && sizeof(E) == 2), "c8 output: fp16 operand pairs");
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (relu) v[i] = v[i] > 0.0f ? v[i] : 0.0f;
                    const cf8::Split4 o = cf8::split4(v);
                    *reinterpret_cast<Quad<_Float16>*>(stage + off) = o.hi;
                    unsigned char* crow = stage + SPART + q * SROWB + (ch & 15);
                    *reinterpret_cast<uint32_t*>(crow + (((ch >> 4) ^ (q & GS::SWZ)) << 4)) = o.l8;
                    *reinterpret_cast<uint32_t*>(crow + (((GS::CPR / 2 + (ch >> 4)) ^ (q & GS::SWZ)) << 4)) = o.h8;
                    continue;
                }
                Quad<E> hi, lo;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (relu) v[i] = v[i] > 0.0f ? v[i] : 0.0f;
                    hi.e[i] = (E)v[i];
                    lo.e[i] = (E)(v[i] - (float)hi.e[i]);
                }
                *reinterpret_cast<Quad<E>*>(stage + off) = hi;
                if (PARTS == 2) *reinterpret_cast<Quad<E>*>(stage + SPART + off) = lo;
            }
        }
        __syncthreads();
        const int n = n0 + bb;
        if (n < n_boards) {
#pragma unroll
            for (int part = 0; part < PARTS; ++part) {
                uint4* dst = reinterpret_cast<uint4*>((part ? yl : yh) + (size_t)n * 90 * C);
                for (int i = tid; i < 90 * GS::CPR; i += NTHR) {
                    const int row = i / GS::CPR, chn = i - row * GS::CPR;
                    dst[i] = *reinterpret_cast<const uint4*>(stage + part * SPART + row * SROWB +
                                                             ((chn ^ (row & GS::SWZ)) << 4));
                }
            }
        }
    }
}

// ---- fp32 activation -> (hi, lo) operand pair, with bias and ReLU (after the 5x5 input convolution) ---------------
template <typename E, int PARTS>
__global__ __launch_bounds__(256) void k_split_bias_act(const float* __restrict__ x, const float* __restrict__ bias,
                                                       E* __restrict__ yh, E* __restrict__ yl, size_t nquad,
                                                       int cquad, int relu)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nquad; i += stride) {
        const float4 a = reinterpret_cast<const float4*>(x)[i];
        float v[4] = {a.x, a.y, a.z, a.w};
        if (bias) {
            const float4 b = reinterpret_cast<const float4*>(bias)[i % (size_t)cquad];
            v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
        }
        Quad<E> hi, lo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (relu) v[k] = v[k] > 0.0f ? v[k] : 0.0f;
            hi.e[k] = (E)v[k];
            lo.e[k] = (E)(v[k] - (float)hi.e[k]);
        }
        reinterpret_cast<Quad<E>*>(yh)[i] = hi;
        if (PARTS == 2) reinterpret_cast<Quad<E>*>(yl)[i] = lo;
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------------
// One function per kernel, each kernel launched from one place; an entry point ends in nn_launched().
struct ConvCall {
    const void *xh, *xl, *wp;
    const float* bias;
    const void *sh, *sl;
    void *yh, *yl;
    float* yf;
    int n, relu;
    hipStream_t st;
};

template <typename E, int C, int P, int PARTS, int MINW = 1>
void launch_conv(const ConvCall& a)
{
    hipLaunchKernelGGL((k_conv3x3<E, C, P, PARTS, MINW>), dim3((unsigned)((a.n + P - 1) / P)), dim3(C / 32 * 64), 0, a.st,
                       (const E*)a.xh, (const E*)a.xl, (const E*)a.wp, a.bias, (const E*)a.sh, (const E*)a.sl, (E*)a.yh,
                       (E*)a.yl, a.yf, a.n, a.relu);
}

template <typename E>
bool dispatch_conv(int channels, int parts, const ConvCall& a)       // false: no kernel for that
{
    if (channels == 128 && parts == 2) launch_conv<E, 128, 2, 2, 1>(a);
    else if (channels == 128 && parts == 1) launch_conv<E, 128, 2, 1, 2>(a);   // 2 workgroups / CU
    else if (channels == 192 && parts == 2) launch_conv<E, 192, 1, 2, 1>(a);
    else if (channels == 192 && parts == 1) launch_conv<E, 192, 2, 1, 1>(a);
    else if (channels == 256 && parts == 2) launch_conv<E, 256, 1, 2>(a);
    else if (channels == 256 && parts == 1) launch_conv<E, 256, 2, 1>(a);
    else if (channels == 32 && parts == 2) launch_conv<E, 32, 2, 2>(a);
    else if (channels == 32 && parts == 1) launch_conv<E, 32, 4, 1>(a);
    else return false;
    return true;
}

template <int C, int P>
void launch_conv_c8(const ConvCall& a)
{
    hipLaunchKernelGGL((k_conv3x3_c8<C, P>), dim3((unsigned)((a.n + P - 1) / P)), dim3(C / 32 * 64), 0, a.st,
                       (const _Float16*)a.xh, (const unsigned char*)a.xl, (const uint4*)a.wp, a.bias, (const _Float16*)a.sh,
                       (const unsigned char*)a.sl, (_Float16*)a.yh, (unsigned char*)a.yl, a.yf, a.n, a.relu);
}

struct InputConvCall {
    const void *planes, *wp;
    const float* bias;
    void *yh, *yl;
    int n, in_planes, relu;
    QueueCtx q;
    hipStream_t st;
};

template <typename E, typename PT, int C, int PARTS, bool C8 = false>
void launch_input_conv(const InputConvCall& a)
{
    constexpr int P = 2;
    const dim3 grid((unsigned)((a.n + P - 1) / P)), block(C / 32 * 64);
    if (a.in_planes <= 16)
        hipLaunchKernelGGL((k_input_conv<E, PT, C, 1, P, PARTS, C8>), grid, block, 0, a.st, (const PT*)a.planes, (const E*)a.wp,
                           a.bias, (E*)a.yh, (E*)a.yl, a.n, a.in_planes, a.relu, a.q.rows, a.q.n_dev);
    else
        hipLaunchKernelGGL((k_input_conv<E, PT, C, 2, P, PARTS, C8>), grid, block, 0, a.st, (const PT*)a.planes, (const E*)a.wp,
                           a.bias, (E*)a.yh, (E*)a.yl, a.n, a.in_planes, a.relu, a.q.rows, a.q.n_dev);
}

template <typename E, typename PT>
bool dispatch_input_conv(int channels, int parts, const InputConvCall& a)
{
    if (channels == 128) { if (parts == 2) launch_input_conv<E, PT, 128, 2>(a); else launch_input_conv<E, PT, 128, 1>(a); }
    else if (channels == 192) { if (parts == 2) launch_input_conv<E, PT, 192, 2>(a); else launch_input_conv<E, PT, 192, 1>(a); }
    else if (channels == 256) { if (parts == 2) launch_input_conv<E, PT, 256, 2>(a); else launch_input_conv<E, PT, 256, 1>(a); }
    else if (channels == 32) { if (parts == 2) launch_input_conv<E, PT, 32, 2>(a); else launch_input_conv<E, PT, 32, 1>(a); }
    else return false;
    return true;
}

template <typename E>
bool dispatch_input_conv_pt(int planes_dtype, int channels, int parts, const InputConvCall& a)
{
    switch (planes_dtype) {
    case CZ_F32: return dispatch_input_conv<E, float>(channels, parts, a);
    case CZ_F16: return dispatch_input_conv<E, _Float16>(channels, parts, a);
    case CZ_BF16: return dispatch_input_conv<E, __bf16>(channels, parts, a);
    case CZ_U8: return dispatch_input_conv<E, unsigned char>(channels, parts, a);
    }
    return false;
}

// one residual block: the operands, the two packed filters, one of the three outputs, the board count on both sides
struct BlockCall {
    const void *xh, *xl, *w1;
    const float* b1;
    const void* w2;
    const float* b2;
    void *yh, *yl;
    float* yf;
    int n, n_cu;
    const int32_t* n_dev;
    hipStream_t st;
};

template <typename E, int C, int PARTS, int P, bool HEADS = false, int CTW = 1>
void launch_resblock(const BlockCall& a, HeadArgs hd = HeadArgs{})
{
    hipLaunchKernelGGL((k_resblock<E, C, PARTS, P, HEADS, CTW>), dim3(nn_grid((a.n + P - 1) / P, a.n_cu)),
                       dim3((C / 32 / CTW + 4) * 64), 0, a.st, (const E*)a.xh, (const E*)a.xl, (const E*)a.w1, a.b1,
                       (const E*)a.w2, a.b2, (E*)a.yh, (E*)a.yl, a.yf, a.n, hd, a.n_dev);
}

template <bool FIRST, bool HEADS, bool C6 = false>
void launch_resblock_c8(const BlockCall& a, HeadArgs hd = HeadArgs{}, FirstArgs fa = FirstArgs{})
{
    hipLaunchKernelGGL((k_resblock_c8<FIRST, HEADS, C6>), dim3(nn_grid(a.n, a.n_cu)), dim3(512), 0, a.st, (const _Float16*)a.xh,
                       (const unsigned char*)a.xl, a.w1, a.b1, a.w2, a.b2, (_Float16*)a.yh, (unsigned char*)a.yl, a.yf, a.n, hd,
                       a.n_dev, fa);
}

template <typename E, bool FIRST = false>
void launch_resblock_pipe(const BlockCall& a, FirstArgs fa = FirstArgs{})
{
    hipLaunchKernelGGL((k_resblock_pipe<E, FIRST>), dim3(nn_grid(a.n, a.n_cu)), dim3(512), 0, a.st, (const E*)a.xh,
                       (const E*)a.xl, (const E*)a.w1, a.b1, (const E*)a.w2, a.b2, (E*)a.yh, (E*)a.yl, a.n, a.n_dev, fa);
}

int g_resblock_pipelined = 1;       // cz_resblock_pipelined(): 128-filter split blocks on k_resblock_pipe

template <typename E>
bool dispatch_resblock(int channels, int parts, const BlockCall& a)
{
    if (channels == 128 && parts == 2 && !a.yf && g_resblock_pipelined)
        // (operand-pair output: the software-pipelined kernel; the last block of a tower -- fp32 / head output --
        //  stays on k_resblock)
        launch_resblock_pipe<E>(a);
    else if (channels == 128 && parts == 2) launch_resblock<E, 128, 2, 1>(a);
    else if (channels == 192 && parts == 2)
        hipLaunchKernelGGL((k_resblock_ip<E, 192>), dim3(nn_grid(a.n, a.n_cu)), dim3(192 / 32 * 64 + ip::COPY_THREADS), 0, a.st,
                           (const E*)a.xh, (const E*)a.xl, (const E*)a.w1, a.b1, (const E*)a.w2, a.b2, (E*)a.yh, (E*)a.yl, a.yf,
                           a.n, a.n_dev);
    else if (channels == 128 && parts == 1) launch_resblock<E, 128, 1, 2>(a);
    else if (channels == 192 && parts == 1) launch_resblock<E, 192, 1, 1>(a);
    // 256 filters, plain operands: two channel tiles per matrix wave (4 + 4 waves), see conv_kloop; the tuning hook's
    // 0 keeps the one-tile schedule (8 + 4 waves) for A/B runs
    else if (channels == 256 && parts == 1 && g_resblock_pipelined) launch_resblock<E, 256, 1, 1, false, 2>(a);
    else if (channels == 256 && parts == 1) launch_resblock<E, 256, 1, 1>(a);
    else return false;
    return true;
}

// 192 filters: that (pair), or one board on six matrix waves (k_resblock_ip_c8; there is no MIX there)
template <int XF, int YF, bool MIX = false>
void launch_ip192(bool pair, const ChainCall& a)
{
    if (pair)
        launch_ip4<192, XF, YF, MIX>(a);
    else
        hipLaunchKernelGGL((k_resblock_ip_c8<192, XF, YF>), dim3(nn_grid(a.n, a.n_cu)), dim3(192 / 32 * 64 + ip::COPY_THREADS), 0,
                           a.st, (const _Float16*)a.xh, (const unsigned char*)a.xc, a.ch, (_Float16*)a.yh, (unsigned char*)a.yc,
                           a.yf, a.n, a.n_dev);
}

// The 192-filter blocks on c8 (CZ_F16C8), on c6 (CZ_F16C6), or behind the input layer's c8 image (CZ_F16C86): as cz_resblock's
// one block (first filter cz_conv3x3_c8_pack_weights', second cz_conv3x3_c6_pack_weights'), or tower_start: as the c6 chain
// that starts the tower, which exists on the four-wave kernel only.
int launch_chain192(const char* name, int dtype, bool tower_start, const ChainCall& a)
{
    const bool pair = nn_ip_pair();
    if (dtype == CZ_F16C86 && tower_start) {
        if (!pair)
            return nn_error(CZ_ERR_ARG, "cz_resblock_chain: CZ_F16C86 (a c6 chain that starts the tower) exists on the four-wave kernel only (CZ_IP_PAIR=0 is set)");
        launch_ip192<1, 1, true>(true, a);
    } else if (dtype == CZ_F16C8) launch_ip192<0, 0>(pair, a);
    else if (dtype == CZ_F16C6) launch_ip192<1, 1>(pair, a);
    else launch_ip192<0, 1>(pair, a);
    return nn_launched(name);
}

}  // namespace

#ifdef CZ_RB_STAMPS
extern "C" int cz_debug_rb_stamps(long long* out32_host)
{
    return hipMemcpyFromSymbol(out32_host, HIP_SYMBOL(g_rb_stamps), sizeof(long long) * 32) == hipSuccess ? CZ_OK : CZ_ERR_HIP;
}
#endif

extern "C" size_t cz_conv3x3_packed_elems(int channels, int parts)
{
    if (channels <= 0 || channels % 32 != 0 || parts < 1 || parts > 2) return 0;
    return (size_t)parts * (size_t)(9 * (channels / 16) + W_PAD_STEPS) * (size_t)(channels / 32) * 64 * 8;
}

extern "C" int cz_conv3x3_pack_weights(const float* w_oihw, int channels, int dtype, int parts, void* out_host)
{
    if (!w_oihw || !out_host || channels <= 0 || channels % 32 != 0 || parts < 1 || parts > 2 ||
        (dtype != CZ_BF16 && dtype != CZ_F16)) {
        czi_set_error("cz_conv3x3_pack_weights: bad argument (channels % 32 == 0, parts 1|2, dtype bf16|f16)");
        return CZ_ERR_ARG;
    }
    const int C = channels, KK = C / 16, CT = C / 32;
    const size_t part_elems = (size_t)(9 * KK + W_PAD_STEPS) * CT * 64 * 8;
    uint16_t* out = (uint16_t*)out_host;
    memset(out, 0, part_elems * parts * sizeof(uint16_t));
    for (int tap = 0; tap < 9; ++tap)
        for (int kk = 0; kk < KK; ++kk)
            for (int ct = 0; ct < CT; ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int o = ct * 32 + (lane & 31);
                        const int c = kk * 16 + (lane >> 5) * 8 + j;
                        const float w = w_oihw[((size_t)o * C + c) * 9 + tap];
                        const size_t idx = ((((size_t)tap * KK + kk) * CT + ct) * 64 + lane) * 8 + j;
                        if (dtype == CZ_BF16) {
                            const uint16_t hi = f32_to_bf16_bits(w);
                            out[idx] = hi;
                            if (parts == 2) out[part_elems + idx] = f32_to_bf16_bits(w - bf16_bits_to_f32(hi));
                        } else {
                            const uint16_t hi = f32_to_f16_bits(w);
                            out[idx] = hi;
                            if (parts == 2) out[part_elems + idx] = f32_to_f16_bits(w - f16_bits_to_f32(hi));
                        }
                    }
    return CZ_OK;
}

// ---- c8 arithmetic (k_conv3x3_c8, k_resblock<C8>): packing and launch ------------------------------------------------------------
namespace {
// float -> OCP e4m3 (bias 7, no infinities, 0x7f = NaN), round to nearest even, saturating at 448
inline uint8_t f32_to_e4m3_bits(float f)
{
    uint32_t fb;
    memcpy(&fb, &f, 4);
    const uint8_t sign = (uint8_t)((fb >> 24) & 0x80);
    float a = fabsf(f);
    if (!(a == a)) return 0x7f;
    if (a >= 448.0f) return sign | 0x7e;
    if (a < ldexpf(1.0f, -10)) return sign;                        // below half the smallest subnormal (2^-9): 0 (tie -> even = 0)
    int e;
    frexpf(a, &e);
    e -= 1;                                                        // a = m * 2^e, m in [1, 2)
    if (e < -6) {                                                  // subnormal: multiples of 2^-9
        const int q = (int)nearbyintf(ldexpf(a, 9));               // 0 .. 8 (8 = the smallest normal, code 0x08)
        return sign | (uint8_t)q;
    }
    int m = (int)nearbyintf(ldexpf(a, 3 - e)) - 8;                 // 0 .. 8
    if (m == 8) { m = 0; e += 1; }
    if (e > 8 || (e == 8 && m > 6)) return sign | 0x7e;
    return sign | (uint8_t)(((e + 7) << 3) | m);
}
// fp32 -> bf6 (e3m2, bias 3, no inf / nan): round to nearest even, saturating at 28 -- v_cvt_scalef32_2xpk16_bf6_f32's rule
inline uint8_t f32_to_bf6_bits(float f)
{
    const uint8_t sgn = std::signbit(f) ? 0x20 : 0;
    float a = fabsf(f);
    if (!(a == a)) return sgn;                                      // (NaN: no encoding; filters never hold one)
    if (a >= 28.0f) return sgn | 0x1F;
    int e;
    frexpf(a, &e);                                                  // a = m 2^e, m in [0.5, 1)
    int ex = e - 1;                                                 // a in [2^ex, 2^(ex + 1))
    if (ex < -2) ex = -2;                                           // subnormals share the smallest normal's step 2^-4
    const float step = ldexpf(1.0f, ex - 2);
    const float qf = nearbyintf(a / step);                          // (default rounding mode: to nearest even)
    const int qi = (int)qf;                                         // 0 .. 8 (8: carries into the next binade)
    if (a < 0.25f) return sgn | (uint8_t)qi;                        // subnormal: code = multiple of 2^-4 (4 -> the first normal)
    int ee = ex + 3, m = qi - 4;
    if (m == 4) { m = 0; ++ee; }
    return sgn | (uint8_t)((ee << 2) | m);
}
inline int pow2_shift_for(float amax, int top)                     // s with amax * 2^s in [2^top, 2^(top + 1))
{
    if (!(amax > 0.0f)) return 0;
    int e;
    frexpf(amax, &e);
    return top - (e - 1);
}
// Per-OUTPUT-CHANNEL shifts of the two correction operands of a filter [C][C][3][3]: out[o] for w, out[C + o] for
// w - f16(w), each the power of two that brings the row's largest magnitude into [2^top, 2^(top + 1)) (clamped to a signed
// byte; an all-zero row: 0).  ints[0], ints[1]: the smallest of each kind (the shift a single scale per tensor would be).
inline void row_shifts(const float* w_oihw, int C, int top, int8_t* out, int32_t* ints)
{
    int min_h = 127, min_l = 127;
    for (int o = 0; o < C; ++o) {
        float wmax = 0.0f, lmax = 0.0f;
        for (size_t i = 0; i < (size_t)C * 9; ++i) {
            const float w = w_oihw[(size_t)o * C * 9 + i], l = w - f16_bits_to_f32(f32_to_f16_bits(w));
            wmax = fabsf(w) > wmax ? fabsf(w) : wmax;
            lmax = fabsf(l) > lmax ? fabsf(l) : lmax;
        }
        int sh = pow2_shift_for(wmax, top), sl = pow2_shift_for(lmax, top);
        sh = sh > 100 ? 100 : (sh < -100 ? -100 : sh);
        sl = sl > 100 ? 100 : (sl < -100 ? -100 : sl);
        out[o] = (int8_t)sh;
        out[C + o] = (int8_t)sl;
        if (wmax > 0.0f && sh < min_h) min_h = sh;
        if (lmax > 0.0f && sl < min_l) min_l = sl;
    }
    ints[0] = min_h == 127 ? 0 : min_h;
    ints[1] = min_l == 127 ? 0 : min_l;
}
}  // namespace

extern "C" size_t cz_conv3x3_c8_packed_bytes(int channels)
{
    if (channels != 128 && channels != 192) return 0;
    const size_t C = channels, KK = C / 16, CT = C / 32, NB = C / 64;
    const size_t main_u4 = (9 * KK + W_PAD_STEPS) * CT * 64, c8_u4 = (9 * NB + 1) * 2 * CT * 2 * 64;
    return (main_u4 + c8_u4 + 1) * 16 + 2 * C;          // fragments, 4 ints, 2 x C per-output-channel shifts (signed bytes)
}

extern "C" int cz_conv3x3_c8_pack_weights(const float* w_oihw, int channels, void* out_host)
{
    if (!w_oihw || !out_host || (channels != 128 && channels != 192)) {
        czi_set_error("cz_conv3x3_c8_pack_weights: bad argument (128 or 192 filters)");
        return CZ_ERR_ARG;
    }
    const int C = channels, KK = C / 16, CT = C / 32, NB = C / 64;
    const size_t main_u4 = (size_t)(9 * KK + W_PAD_STEPS) * CT * 64, c8_u4 = (size_t)(9 * NB + 1) * 2 * CT * 2 * 64;
    memset(out_host, 0, (main_u4 + c8_u4 + 1) * 16 + 2 * (size_t)C);
    uint16_t* hi = (uint16_t*)out_host;
    uint8_t* c8p = (uint8_t*)out_host + main_u4 * 16;
    int32_t* sc = (int32_t*)((uint8_t*)out_host + (main_u4 + c8_u4) * 16);
    int8_t* row_sh = (int8_t*)(sc + 4);                  // per output channel: shift of e4m3(w), then (row_sh + C) of e4m3(w - f16(w))
    row_shifts(w_oihw, C, 7, row_sh, sc);                // largest magnitude of a row in [128, 256): below 448
    for (int tap = 0; tap < 9; ++tap)
        for (int ct = 0; ct < CT; ++ct)
            for (int lane = 0; lane < 64; ++lane) {
                const int o = ct * 32 + (lane & 31);
                for (int kk = 0; kk < KK; ++kk)
                    for (int j = 0; j < 8; ++j) {
                        const int c = kk * 16 + (lane >> 5) * 8 + j;
                        const float w = w_oihw[((size_t)o * C + c) * 9 + tap];
                        hi[((((size_t)tap * KK + kk) * CT + ct) * 64 + lane) * 8 + j] = f32_to_f16_bits(w);
                    }
                for (int b = 0; b < NB; ++b)
                    for (int q = 0; q < 2; ++q)
                        for (int j = 0; j < 32; ++j) {
                            const int c = b * 64 + (lane >> 5) * 32 + j;
                            const float w = w_oihw[((size_t)o * C + c) * 9 + tap];
                            const float v = q == 0 ? ldexpf(w, row_sh[o]) : ldexpf(w - f16_bits_to_f32(f32_to_f16_bits(w)), row_sh[C + o]);
                            const size_t u4 = ((((size_t)(tap * NB + b) * 2 + q) * CT + ct) * 2 + j / 16) * 64 + lane;
                            c8p[u4 * 16 + j % 16] = f32_to_e4m3_bits(v);
                        }
            }
    return CZ_OK;
}

// The same filter for the c6 arithmetic (k_resblock_c8<.., C6>): fp16 fragments as above; the correction pieces in bf6,
// 24 bytes per lane -- a 16-byte head where the e4m3 piece's first half sits, the 8-byte tails densely behind the heads of
// a (block, kind, wave) group -- with element e of lane (row, half) = input channel 64 b + 32 half + 8 (e >> 3) +
// ((e >> 1) & 3) + 4 (e & 1) (the order the kernels' conversion instruction gives the activations).  Trailing ints:
// the two filter shifts (largest magnitude in [8, 16): bf6 saturates at 28), then x_exp / y_exp: the exponents k of the
// activation image this convolution reads and of the one it writes (x_hi6 = bf6(x 2^-k); 2^k 28 >= max |x|).
extern "C" int cz_conv3x3_c6_pack_weights(const float* w_oihw, int channels, int x_exp, int y_exp, void* out_host)
{
    if (!w_oihw || !out_host || (channels != 128 && channels != 192) || x_exp < -100 || x_exp > 100 ||
        ((y_exp < -100 || y_exp > 100) && y_exp != CZ_C6_OUT_C8)) {
        czi_set_error("cz_conv3x3_c6_pack_weights: bad argument (128 or 192 filters; image exponents within +-100, or y_exp 127 = c8 output)");
        return CZ_ERR_ARG;
    }
    const int C = channels, KK = C / 16, CT = C / 32, NB = C / 64;
    const size_t main_u4 = (size_t)(9 * KK + W_PAD_STEPS) * CT * 64, c8_u4 = (size_t)(9 * NB + 1) * 2 * CT * 2 * 64;
    memset(out_host, 0, (main_u4 + c8_u4 + 1) * 16 + 2 * (size_t)C);
    uint16_t* hi = (uint16_t*)out_host;
    uint8_t* c6p = (uint8_t*)out_host + main_u4 * 16;
    int32_t* sc = (int32_t*)((uint8_t*)out_host + (main_u4 + c8_u4) * 16);
    int8_t* row_sh = (int8_t*)(sc + 4);
    row_shifts(w_oihw, C, 3, row_sh, sc);                // largest magnitude of a row in [8, 16): bf6 saturates at 28
    sc[2] = x_exp;
    sc[3] = y_exp;
    for (int tap = 0; tap < 9; ++tap)
        for (int ct = 0; ct < CT; ++ct)
            for (int lane = 0; lane < 64; ++lane) {
                const int o = ct * 32 + (lane & 31);
                for (int kk = 0; kk < KK; ++kk)
                    for (int j = 0; j < 8; ++j) {
                        const int c = kk * 16 + (lane >> 5) * 8 + j;
                        const float w = w_oihw[((size_t)o * C + c) * 9 + tap];
                        hi[((((size_t)tap * KK + kk) * CT + ct) * 64 + lane) * 8 + j] = f32_to_f16_bits(w);
                    }
                for (int b = 0; b < NB; ++b)
                    for (int q = 0; q < 2; ++q) {
                        uint8_t piece[24] = {0};
                        for (int e = 0; e < 32; ++e) {
                            const int c = b * 64 + (lane >> 5) * 32 + 8 * (e >> 3) + ((e >> 1) & 3) + 4 * (e & 1);
                            const float w = w_oihw[((size_t)o * C + c) * 9 + tap];
                            const float v = q == 0 ? ldexpf(w, row_sh[o]) : ldexpf(w - f16_bits_to_f32(f32_to_f16_bits(w)), row_sh[C + o]);
                            const uint32_t code = f32_to_bf6_bits(v);
                            const int bit = 6 * e;
                            piece[bit >> 3] |= (uint8_t)(code << (bit & 7));
                            if ((bit & 7) > 2) piece[(bit >> 3) + 1] |= (uint8_t)(code >> (8 - (bit & 7)));
                        }
                        uint8_t* grp = c6p + ((((size_t)(tap * NB + b) * 2 + q) * CT + ct) * 2) * 64 * 16;    // 2 KB per (block, kind, wave)
                        memcpy(grp + (size_t)lane * 16, piece, 16);
                        memcpy(grp + 1024 + (size_t)lane * 8, piece + 16, 8);
                    }
            }
    return CZ_OK;
}

extern "C" int cz_conv3x3_c8(const void* x_hi, const void* x_c8, const void* w_packed, const float* bias,
                             const void* skip_hi, const void* skip_c8, void* y_hi, void* y_c8, float* y_f32,
                             int n_boards, int channels, int relu, void* stream)
{
    if (n_boards < 0 || !x_hi || !x_c8 || !w_packed || !bias || (channels != 128 && channels != 192) ||
        (!y_f32 && (!y_hi || !y_c8)) || (skip_hi && !skip_c8))
        return nn_error(CZ_ERR_ARG, "cz_conv3x3_c8: bad argument (128 or 192 filters; output: y_f32, or the operand pair y_hi + y_c8)");
    if (n_boards == 0) return CZ_OK;
    const ConvCall a{x_hi, x_c8, w_packed, bias, skip_hi, skip_c8, y_hi, y_c8, y_f32, n_boards, relu, (hipStream_t)stream};
    if (channels == 128) launch_conv_c8<128, 2>(a);
    else launch_conv_c8<192, 1>(a);
    return nn_launched("cz_conv3x3_c8");
}

extern "C" int cz_conv3x3(const void* x_hi, const void* x_lo, const void* w_packed, const float* bias,
                          const void* skip_hi, const void* skip_lo, void* y_hi, void* y_lo, float* y_f32,
                          int n_boards, int channels, int dtype, int parts, int relu, void* stream)
{
    if (n_boards < 0 || !w_packed || !bias || !x_hi || (parts == 2 && !x_lo) || (parts != 1 && parts != 2) ||
        (!y_f32 && (!y_hi || (parts == 2 && !y_lo))) || (skip_hi && parts == 2 && !skip_lo))
        return nn_error(CZ_ERR_ARG, "cz_conv3x3: bad argument");
    if (n_boards == 0) return CZ_OK;
    const ConvCall a{x_hi, x_lo, w_packed, bias, skip_hi, skip_lo, y_hi, y_lo, y_f32, n_boards, relu, (hipStream_t)stream};
    if (!(dtype == CZ_BF16 ? dispatch_conv<__bf16>(channels, parts, a) : dtype == CZ_F16 && dispatch_conv<_Float16>(channels, parts, a)))
        return nn_error(CZ_ERR_ARG, "cz_conv3x3: unsupported channels / dtype (channels 32|128|192|256, bf16|f16)");
    return nn_launched("cz_conv3x3");
}

extern "C" size_t cz_input_conv_packed_elems(int channels, int in_planes, int parts)
{
    if (channels <= 0 || channels % 32 != 0 || parts < 1 || parts > 2 || in_planes < 1 || in_planes > 32) return 0;
    const int ic16 = (in_planes + 15) / 16;
    return (size_t)parts * (size_t)(25 + 3) * ic16 * (size_t)(channels / 32) * 64 * 8;
}

extern "C" int cz_input_conv_pack_weights(const float* w_oihw, int channels, int in_planes, int dtype, int parts,
                                          void* out_host)
{
    if (!w_oihw || !out_host || cz_input_conv_packed_elems(channels, in_planes, parts) == 0 ||
        (dtype != CZ_BF16 && dtype != CZ_F16)) {
        czi_set_error("cz_input_conv_pack_weights: bad argument");
        return CZ_ERR_ARG;
    }
    const int CT = channels / 32, ic16 = (in_planes + 15) / 16;
    const size_t part_elems = (size_t)(25 + 3) * ic16 * CT * 64 * 8;
    uint16_t* out = (uint16_t*)out_host;
    memset(out, 0, part_elems * parts * sizeof(uint16_t));
    for (int tap = 0; tap < 25; ++tap)
        for (int g = 0; g < ic16; ++g)
            for (int ct = 0; ct < CT; ++ct)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 8; ++j) {
                        const int o = ct * 32 + (lane & 31);
                        const int c = g * 16 + (lane >> 5) * 8 + j;
                        if (c >= in_planes) continue;
                        const float w = w_oihw[((size_t)o * in_planes + c) * 25 + tap];
                        const size_t idx = ((((size_t)tap * ic16 + g) * CT + ct) * 64 + lane) * 8 + j;
                        if (dtype == CZ_BF16) {
                            const uint16_t hi = f32_to_bf16_bits(w);
                            out[idx] = hi;
                            if (parts == 2) out[part_elems + idx] = f32_to_bf16_bits(w - bf16_bits_to_f32(hi));
                        } else {
                            const uint16_t hi = f32_to_f16_bits(w);
                            out[idx] = hi;
                            if (parts == 2) out[part_elems + idx] = f32_to_f16_bits(w - f16_bits_to_f32(hi));
                        }
                    }
    return CZ_OK;
}

namespace {
// cz_input_conv and cz_input_conv_q
int input_conv(QueueCtx q, const void* planes, int planes_dtype, int in_planes, const void* w_packed, const float* bias,
               void* y_hi, void* y_lo, int n_boards, int channels, int dtype, int parts, int relu, void* stream)
{
    if (n_boards < 0 || !planes || !w_packed || !bias || !y_hi || (parts == 2 && !y_lo) || (parts != 1 && parts != 2) ||
        in_planes < 1 || in_planes > 32)
        return nn_error(CZ_ERR_ARG, "cz_input_conv: bad argument");
    if (n_boards == 0) return CZ_OK;
    const InputConvCall a{planes, w_packed, bias, y_hi, y_lo, n_boards, in_planes, relu, q, (hipStream_t)stream};
    bool ok = false;
    if (dtype == CZ_BF16)
        ok = dispatch_input_conv_pt<__bf16>(planes_dtype, channels, parts, a);
    else if (dtype == CZ_F16)
        ok = dispatch_input_conv_pt<_Float16>(planes_dtype, channels, parts, a);
    else if (dtype == CZ_F16C8 && (channels == 128 || channels == 192) && parts == 2 &&
             (planes_dtype == CZ_U8 || planes_dtype == CZ_F32)) {
        // f16-split filters (cz_input_conv_pack_weights with CZ_F16), output = the c8 operand pair (y_lo = the c8 image)
        ok = true;
        if (channels == 128 && planes_dtype == CZ_U8) launch_input_conv<_Float16, unsigned char, 128, 2, true>(a);
        else if (channels == 128) launch_input_conv<_Float16, float, 128, 2, true>(a);
        else if (planes_dtype == CZ_U8) launch_input_conv<_Float16, unsigned char, 192, 2, true>(a);
        else launch_input_conv<_Float16, float, 192, 2, true>(a);
    }
    if (!ok) return nn_error(CZ_ERR_ARG, "cz_input_conv: unsupported channels / dtype");
    return nn_launched("cz_input_conv");
}

// cz_resblock_heads and cz_resblock_heads_q
int resblock_heads(const int32_t* n_dev, const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1,
                   const void* w2_packed, const float* bias2, const float* head_w, const float* head_b, float* policy_feat,
                   float* value_feat, int n_boards, int channels, int dtype, int n_policy, int n_value, void* stream)
{
    if (n_boards < 0 || !x_hi || !x_lo || !w1_packed || !w2_packed || !bias1 || !bias2 || !head_w || !head_b ||
        !policy_feat || !value_feat || n_policy < 1 || n_value < 1 || n_policy + n_value != 6)
        return nn_error(CZ_ERR_ARG, "cz_resblock_heads: bad argument (split operands; n_policy + n_value == 6)");
    if (n_boards == 0) return CZ_OK;
    if (channels != 128 || (dtype != CZ_BF16 && dtype != CZ_F16 && dtype != CZ_F16C8 && dtype != CZ_F16C6))
        return nn_error(CZ_ERR_ARG, "cz_resblock_heads: 128 filters, bf16 / f16 split operands only (use cz_resblock + cz_head_convs)");
    const int n_cu = nn_cu_count("cz_resblock_heads");
    if (n_cu < 0) return CZ_ERR_HIP;
    const HeadArgs hd{head_w, head_b, policy_feat, value_feat, n_policy};
    const BlockCall a{x_hi, x_lo, w1_packed, bias1, w2_packed, bias2, nullptr, nullptr, nullptr, n_boards, n_cu, n_dev,
                      (hipStream_t)stream};
    if (dtype == CZ_BF16) launch_resblock<__bf16, 128, 2, 1, true>(a, hd);
    else if (dtype == CZ_F16C8) launch_resblock_c8<false, true>(a, hd);
    else if (dtype == CZ_F16C6) launch_resblock_c8<false, true, true>(a, hd);
    else launch_resblock<_Float16, 128, 2, 1, true>(a, hd);
    return nn_launched("cz_resblock_heads");
}

// cz_resblock and cz_resblock_q
int resblock(const int32_t* n_dev, const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1,
             const void* w2_packed, const float* bias2, void* y_hi, void* y_lo, float* y_f32, int n_boards, int channels,
             int dtype, int parts, void* stream)
{
    if (n_boards < 0 || !x_hi || !w1_packed || !w2_packed || !bias1 || !bias2 || (parts != 1 && parts != 2) ||
        (parts == 2 && (!x_lo || (!y_f32 && (!y_hi || !y_lo)))) || (parts == 1 && (!y_hi || y_f32)))
        return nn_error(CZ_ERR_ARG, "cz_resblock: bad argument (parts = 1 writes y_hi only; y_f32 needs parts = 2)");
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_resblock");
    if (n_cu < 0) return CZ_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    const BlockCall a{x_hi, x_lo, w1_packed, bias1, w2_packed, bias2, y_hi, y_lo, y_f32, n_boards, n_cu, n_dev, st};
    bool ok = true;
    if (dtype == CZ_BF16) ok = dispatch_resblock<__bf16>(channels, parts, a);
    else if (dtype == CZ_F16) ok = dispatch_resblock<_Float16>(channels, parts, a);
    else if (dtype == CZ_F16C8 && channels == 128 && parts == 2) launch_resblock_c8<false, false>(a);
    else if (dtype == CZ_F16C6 && channels == 128 && parts == 2) launch_resblock_c8<false, false, true>(a);
    else if ((dtype == CZ_F16C8 || dtype == CZ_F16C6 || dtype == CZ_F16C86) && channels == 192 && parts == 2) {
        // 192 filters: the two-image in-place block, as a chain of one
        BlockChain<ip::MAX_BLOCKS> ch{};
        fill_chain(ch, "cz_resblock", 1, &w1_packed, &bias1, &w2_packed, &bias2);
        return launch_chain192("cz_resblock", dtype, false, ChainCall{x_hi, x_lo, ch, y_hi, y_lo, y_f32, n_boards, n_cu, n_dev, st});
    } else ok = false;
    if (!ok)
        return nn_error(CZ_ERR_ARG, "cz_resblock: supported: 128 / 192 filters (split or plain operands), 256 filters (plain), bf16 / f16; "
                                    "use cz_conv3x3 otherwise");
    return nn_launched("cz_resblock");
}
}  // namespace

extern "C" int cz_input_conv(const void* planes, int planes_dtype, int in_planes, const void* w_packed,
                             const float* bias, void* y_hi, void* y_lo, int n_boards, int channels, int dtype,
                             int parts, int relu, void* stream)
{
    return input_conv(QueueCtx{nullptr, nullptr}, planes, planes_dtype, in_planes, w_packed, bias, y_hi, y_lo, n_boards, channels,
                      dtype, parts, relu, stream);
}

extern "C" int cz_resblock_heads(const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1,
                                 const void* w2_packed, const float* bias2, const float* head_w, const float* head_b,
                                 float* policy_feat, float* value_feat, int n_boards, int channels, int dtype,
                                 int n_policy, int n_value, void* stream)
{
    return resblock_heads(nullptr, x_hi, x_lo, w1_packed, bias1, w2_packed, bias2, head_w, head_b, policy_feat, value_feat,
                          n_boards, channels, dtype, n_policy, n_value, stream);
}

extern "C" int cz_resblock(const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1,
                           const void* w2_packed, const float* bias2, void* y_hi, void* y_lo, float* y_f32,
                           int n_boards, int channels, int dtype, int parts, void* stream)
{
    return resblock(nullptr, x_hi, x_lo, w1_packed, bias1, w2_packed, bias2, y_hi, y_lo, y_f32, n_boards, channels, dtype, parts,
                    stream);
}

// ---- compact evaluation queue: the same kernels with a device-side board count (and a row gather in the input layer) ----
extern "C" int cz_input_conv_q(const void* planes, int planes_dtype, int in_planes, const void* w_packed,
                               const float* bias, void* y_hi, void* y_lo, int n_boards, int channels, int dtype,
                               int parts, int relu, const int32_t* rows, const int32_t* n_dev, void* stream)
{
    return input_conv(QueueCtx{rows, n_dev}, planes, planes_dtype, in_planes, w_packed, bias, y_hi, y_lo, n_boards, channels,
                      dtype, parts, relu, stream);
}

extern "C" int cz_resblock_q(const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1,
                             const void* w2_packed, const float* bias2, void* y_hi, void* y_lo, float* y_f32,
                             int n_boards, int channels, int dtype, int parts, const int32_t* n_dev, void* stream)
{
    return resblock(n_dev, x_hi, x_lo, w1_packed, bias1, w2_packed, bias2, y_hi, y_lo, y_f32, n_boards, channels, dtype, parts,
                    stream);
}

extern "C" int cz_resblock_heads_q(const void* x_hi, const void* x_lo, const void* w1_packed, const float* bias1,
                                   const void* w2_packed, const float* bias2, const float* head_w, const float* head_b,
                                   float* policy_feat, float* value_feat, int n_boards, int channels, int dtype,
                                   int n_policy, int n_value, const int32_t* n_dev, void* stream)
{
    return resblock_heads(n_dev, x_hi, x_lo, w1_packed, bias1, w2_packed, bias2, head_w, head_b, policy_feat, value_feat,
                          n_boards, channels, dtype, n_policy, n_value, stream);
}

// n_blocks (1 .. 12) consecutive residual blocks of a 192-filter tower on ONE staged arithmetic in one launch (k_resblock_ip_c8's
// chain): dtype CZ_F16C8 (c8 blocks) or CZ_F16C6 (c6 blocks behind the tower's first one).  y_f32 != NULL: the last block writes
// fp32 instead of the operand pair.
extern "C" int cz_resblock_chain(const void* x_hi, const void* x_img, int n_blocks, const void* const* w1_packed,
                                 const float* const* bias1, const void* const* w2_packed, const float* const* bias2, void* y_hi,
                                 void* y_img, float* y_f32, int n_boards, int channels, int dtype, const int32_t* n_dev,
                                 void* stream)
{
    const bool pairs = dtype == CZ_F16 || dtype == CZ_BF16;     // (hi, lo) pair blocks: x_img / y_img are the lo tensors
    if (n_boards < 0 || !x_hi || !x_img || !w1_packed || !w2_packed || !bias1 || !bias2 || n_blocks < 1 ||
        n_blocks > ip::MAX_BLOCKS || channels != 192 || (dtype != CZ_F16C8 && dtype != CZ_F16C6 && dtype != CZ_F16C86 && !pairs) ||
        (!y_f32 && (!y_hi || !y_img)))
        return nn_error(CZ_ERR_ARG, "cz_resblock_chain: bad argument (192 filters, 1 .. 12 blocks, dtype CZ_F16C8 / CZ_F16C6 / CZ_F16C86 with y_f32 or y_hi + y_img, "
                                    "or CZ_F16 / CZ_BF16 pair blocks with y_f32 or y_hi + y_lo)");
    BlockChain<ip::MAX_BLOCKS> ch{};
    if (!fill_chain(ch, "cz_resblock_chain", n_blocks, w1_packed, bias1, w2_packed, bias2)) return CZ_ERR_ARG;
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_resblock_chain");
    if (n_cu < 0) return CZ_ERR_HIP;
    if (pairs)
        return czi_pairs4_launch("cz_resblock_chain", x_hi, x_img, &ch, y_hi, y_img, nullptr, nullptr, nullptr, nullptr, 0, n_boards,
                                 192, dtype, n_cu, n_dev, stream, y_f32);
    return launch_chain192("cz_resblock_chain", dtype, true,
                           ChainCall{x_hi, x_img, ch, y_hi, y_img, y_f32, n_boards, n_cu, n_dev, (hipStream_t)stream});
}

// n_blocks (1 .. 24) consecutive residual blocks of a 256-filter tower on plain fp16 / bf16 operands in one launch
// (k_tower_plain2: a pair of boards per workgroup, one LDS image per board): the `deep` 20 x 256 configuration is ONE launch.  Filters: cz_conv3x3_pack_weights(parts = 1).
extern "C" int cz_tower_plain(const void* x, int n_blocks, const void* const* w1_packed, const float* const* bias1,
                              const void* const* w2_packed, const float* const* bias2, void* y, int n_boards, int channels,
                              int dtype, const int32_t* n_dev, void* stream)
{
    if (n_boards < 0 || !x || !y || !w1_packed || !w2_packed || !bias1 || !bias2 || n_blocks < 1 || n_blocks > pl::MAX_BLOCKS ||
        channels != 256 || (dtype != CZ_F16 && dtype != CZ_BF16))
        return nn_error(CZ_ERR_ARG, "cz_tower_plain: bad argument (256 filters, plain f16 / bf16 operands, 1 .. 24 blocks)");
    BlockChain<pl::MAX_BLOCKS> ch{};
    if (!fill_chain(ch, "cz_tower_plain", n_blocks, w1_packed, bias1, w2_packed, bias2)) return CZ_ERR_ARG;
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_tower_plain");
    if (n_cu < 0) return CZ_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(nn_grid((n_boards + 1) / 2, n_cu)), block(256 / 32 / 2 * 64);
    if (dtype == CZ_F16)
        hipLaunchKernelGGL((k_tower_plain2<_Float16, 256, 2>), grid, block, 0, st, (const _Float16*)x, ch, (_Float16*)y, n_boards, n_dev);
    else
        hipLaunchKernelGGL((k_tower_plain2<__bf16, 256, 2>), grid, block, 0, st, (const __bf16*)x, ch, (__bf16*)y, n_boards, n_dev);
    return nn_launched("cz_tower_plain");
}

// The input layer and the first residual block in one launch (k_resblock_pipe<FIRST>): the 5 x 5 input convolution of
// the one-hot feature planes is a gather over the occupied squares, done by the block's copy waves.
// With the positions' occupancy boards handed in (masks [n][96] uint32 DEVICE, word = plane position, bit c = plane c shows
// a piece there: what cz_search_leaf_masks makes the search kernel write beside the planes) the copy waves skip deriving them
// from the 1260 plane bytes, and the planes are not read at all.  masks = NULL: exactly cz_input_resblock.
extern "C" int cz_input_resblock_m(const void* planes_u8, const uint32_t* masks, int in_planes, const float* in_table,
                                   const float* in_bias, const void* w1_packed, const float* bias1, const void* w2_packed,
                                   const float* bias2, void* y_hi, void* y_lo, int n_boards, int channels, int dtype,
                                   const int32_t* rows, const int32_t* n_dev, void* stream)
{
    if (n_boards < 0 || (!planes_u8 && !masks) || !in_table || !in_bias || !w1_packed || !w2_packed || !bias1 || !bias2 || !y_hi ||
        !y_lo || in_planes < 1 || in_planes > 32 || (in_planes * 90) % 4 != 0)
        return nn_error(CZ_ERR_ARG, "cz_input_resblock: bad argument (u8 planes, in_planes even and <= 32)");
    if (channels != 128 || (dtype != CZ_BF16 && dtype != CZ_F16 && dtype != CZ_F16C8 && dtype != CZ_F16C6))
        return nn_error(CZ_ERR_ARG, "cz_input_resblock: 128 filters; bf16 / f16 split operands or the c8 / c6 pair (use cz_input_conv + cz_resblock)");
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_input_resblock");
    if (n_cu < 0) return CZ_ERR_HIP;
    // 6 of the ~12-16 term rounds of a board under K loop 1, the rest under K loop 2: measured on one box, extra time of
    // the launch against an inner block's: 0 rounds +0.43 ms, 3: +0.26, 6: +0.14, 9: +0.22 (window 2 also drains the result)
    // (tuning hook for A/B runs of the fused input layer: CZ_FIRST_W1_ROUNDS, read once per process)
    static const char* const w1_env = getenv("CZ_FIRST_W1_ROUNDS");
    static const int w1_rounds = w1_env ? atoi(w1_env) : 6;
    const FirstArgs fa{(const unsigned char*)planes_u8, in_table, in_bias, rows, masks, in_planes, w1_rounds};
    const BlockCall a{nullptr, nullptr, w1_packed, bias1, w2_packed, bias2, y_hi, y_lo, nullptr, n_boards, n_cu, n_dev,
                      (hipStream_t)stream};
    // CZ_F16C6: y_lo = a c6 image; w1: cz_conv3x3_c8_pack_weights' (the gather's image is c8), w2: ..._c6_...
    // CZ_F16C8: y_lo = the c8 image, the filters are cz_conv3x3_c8_pack_weights' (k_resblock_c8<FIRST>)
    if (dtype == CZ_F16C6) launch_resblock_c8<true, false, true>(a, HeadArgs{}, fa);
    else if (dtype == CZ_F16C8) launch_resblock_c8<true, false>(a, HeadArgs{}, fa);
    else if (dtype == CZ_BF16) launch_resblock_pipe<__bf16, true>(a, fa);
    else launch_resblock_pipe<_Float16, true>(a, fa);
    return nn_launched("cz_input_resblock");
}

extern "C" int cz_input_resblock(const void* planes_u8, int in_planes, const float* in_table, const float* in_bias,
                                 const void* w1_packed, const float* bias1, const void* w2_packed, const float* bias2,
                                 void* y_hi, void* y_lo, int n_boards, int channels, int dtype, const int32_t* rows,
                                 const int32_t* n_dev, void* stream)
{
    return cz_input_resblock_m(planes_u8, nullptr, in_planes, in_table, in_bias, w1_packed, bias1, w2_packed, bias2, y_hi, y_lo,
                               n_boards, channels, dtype, rows, n_dev, stream);
}

// test / tuning hook: 1 (default) = 128-filter split residual blocks with operand-pair output run on the
// software-pipelined kernel (k_resblock_pipe), 0 = on k_resblock.  Returns the previous setting.
extern "C" int cz_resblock_pipelined(int enable)
{
    const int old = g_resblock_pipelined;
    if (enable >= 0) g_resblock_pipelined = enable ? 1 : 0;
    return old;
}

template <typename E, int PARTS>
static void launch_split(unsigned blocks, hipStream_t st, const float* x, const float* bias, void* y_hi, void* y_lo, size_t nquad,
                         int cquad, int relu)
{
    hipLaunchKernelGGL((k_split_bias_act<E, PARTS>), dim3(blocks), dim3(256), 0, st, x, bias, (E*)y_hi, (E*)y_lo, nquad, cquad, relu);
}

extern "C" int cz_split_bias_act(const float* x, const float* bias, void* y_hi, void* y_lo, size_t n_elems,
                                 int channels, int dtype, int parts, int relu, void* stream)
{
    if (!x || !y_hi || (parts == 2 && !y_lo) || (parts != 1 && parts != 2) || channels <= 0 || channels % 4 != 0 ||
        n_elems % (size_t)channels != 0 || (dtype != CZ_BF16 && dtype != CZ_F16))
        return nn_error(CZ_ERR_ARG, "cz_split_bias_act: bad argument");
    if (n_elems == 0) return CZ_OK;
    hipStream_t st = (hipStream_t)stream;
    const size_t nquad = n_elems / 4;
    const size_t tiles = (nquad + 255) / 256;
    const unsigned blocks = (unsigned)(tiles < 256 * 16 ? tiles : 256 * 16);
    const int cquad = channels / 4;
    if (dtype == CZ_BF16 && parts == 2) launch_split<__bf16, 2>(blocks, st, x, bias, y_hi, y_lo, nquad, cquad, relu);
    else if (dtype == CZ_BF16) launch_split<__bf16, 1>(blocks, st, x, bias, y_hi, y_lo, nquad, cquad, relu);
    else if (parts == 2) launch_split<_Float16, 2>(blocks, st, x, bias, y_hi, y_lo, nquad, cquad, relu);
    else launch_split<_Float16, 1>(blocks, st, x, bias, y_hi, y_lo, nquad, cquad, relu);
    return nn_launched("cz_split_bias_act");
}
