// xq_heads.hip -- the dense tail of the policy / value heads as hand-written MFMA kernels (gfx950).
//
// Reference (cchess_alphazero/agent/model.py:56-66, after the two 1x1 head convolutions):
//     policy:  Flatten -> Dense(2086, softmax)
//     value:   Flatten -> Dense(256, relu) -> Dense(1, tanh)
// Round 2 ran these on hipBLASLt fp32 GEMMs + PyTorch's softmax / clamp / tanh kernels: 0.87 ms of a 31 ms self-play
// round at 32 768 positions (an fp32 GEMM at the fp32 matrix rate, then 546 MB of softmax traffic), eight launches.
// Here:
//   k_fc_tile<POLICY>   logits[n][2086] = feat[n][F] . W^T + b for a tile of 64 positions per workgroup, written
//                       un-normalised, with the row's running (max, sum of exp) kept per lane -- no cross-lane work in
//                       the loop: the positions are the COLUMNS of the MFMA, so a lane owns one position
//   k_policy_normalize  p = exp(logit - max) / sum in place (one streaming pass, rows of 8344 bytes, 8-byte accesses)
//   k_fc_tile<VALUE>    hidden = relu(feat . W1^T + b1) stays in the accumulators, value = tanh(hidden . w2 + b2)
//   k_fc_tile<WDL>      the same hidden layer against w2[3][n_hidden]: three logits (win, draw, loss) per position, a
//                       max-subtracted softmax in fp32, value = (e_W - e_L) / ((e_W + e_L) + e_D) (cz_heads_tail_wdl)
//   k_fc_tile<VALUE_ML / WDL_ML>  either of the two with one more row of w2 behind the head's own: the moves-left output
//                       x = hidden . w2[ml] + b2[ml], written raw (cz_heads_tail_ml); value and wdl keep their bits
// Arithmetic: the same split-operand scheme as the tower (xq_conv.hip): every fp32 operand is a (hi, lo) pair of 2-byte
// values, a product is accumulated as w_hi x_hi + w_lo x_hi + w_hi x_lo in fp32 by v_mfma_f32_32x32x16_{bf16,f16}.
// dtype CZ_BF16: dropped term and representation error 2^-17 relative per product; CZ_F16 (round 4, what the network
// uses unless bf16x3 was asked for): (hi, lo) fp16 pairs hold 22 bits where fp16's range holds the lo part (features are
// O(1), fp16 subnormal inputs are honoured by the matrix unit -- tests/test_gpu_f16x3.py), 2^-21 class, same cost.  Order: K-steps of 16 features in index
// order, the three terms of a step in the order above; the softmax statistics are accumulated per lane over its label
// tiles in index order, combined across the two half-waves and the four waves of a position tile in a fixed order.
// Weights are packed on the host in fragment order (cz_fc_pack_weights); they stream from L2 (3 MB for the policy
// layer), the features of the tile sit in LDS as the B operand.
// The compact evaluation queue's device-side count is honoured (n_dev): rows beyond it are not computed or written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/czero.h"
#include "xq_nn_launch.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

template <typename E> struct FcMma;
template <> struct FcMma<__bf16> {
    static __device__ __forceinline__ f32x16 mma(uint4 a, uint4 b, f32x16 c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct FcMma<_Float16> {
    static __device__ __forceinline__ f32x16 mma(uint4 a, uint4 b, f32x16 c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};

constexpr int TILE_ROWS = 64;         // positions per workgroup pass (two MFMA column tiles)
constexpr int FC_THREADS = 512;       // 8 waves: wave w -> position tile w & 1, label tiles (w >> 1) mod 4
constexpr int FC_PAD_STEPS = 2;       // zero K-steps appended per label tile (the prefetch reads one step ahead)
constexpr int FC_MAX_KSTEPS = 24;     // features per position <= 384 (the reference's heads: 2 or 4 filters x 90 squares)
constexpr int FC_IMG_BYTES = 2 * TILE_ROWS * (FC_MAX_KSTEPS * 32 + 16);
constexpr int FC_RED_BYTES = 2 * 256 * (int)sizeof(float);
constexpr int FC_STAGE_ROW = 144;     // bytes per position row of a wave's logit staging tile (32 floats + 16 B: odd in 16-B units)
constexpr int FC_STAGE_BYTES = 32 * FC_STAGE_ROW;            // per wave
constexpr int FC_LDS_BYTES = FC_IMG_BYTES + FC_RED_BYTES + (FC_THREADS / 64) * FC_STAGE_BYTES;

enum FcMode { FC_POLICY = 0, FC_VALUE = 1, FC_WDL = 2, FC_VALUE_ML = 3, FC_WDL_ML = 4 };

struct FcArgs {
    const float* feat;        // [n][F]
    const void* wp;           // packed weights [label tiles][ksteps + pad][2 parts][64 lanes][8]
    const float* bias;        // [n_out]
    int F, ksteps, n_out, n_tiles;
    // policy
    float* logits;            // [n][n_out]
    float2* stats;            // [n] (max, sum exp)
    // value
    const float* w2;          // [n_out]
    float b2;
    float* value;             // [n]
};

// FC_WDL's arguments: w2 is [3][n_out] (win, draw, loss), b2 the win bias.  A type of its own, so that the other two modes
// keep the kernel arguments they had.
struct FcArgsWdl : FcArgs {
    float b2_draw, b2_loss;
    float* wdl;               // [n][3] probabilities, or NULL
};
template <int MODE> struct FcArgsOf { typedef FcArgs T; };
template <> struct FcArgsOf<FC_WDL> { typedef FcArgsWdl T; };
// FC_WDL combines three sums per position: the third lies behind `red`, in the logit staging tiles only FC_POLICY uses
static_assert(3 * 256 * (int)sizeof(float) <= FC_RED_BYTES + FC_STAGE_BYTES, "the third WDL sum fits the first staging tile");

// The moves-left modes' arguments (cz_heads_tail_ml): the value head's own fields as they are (FC_VALUE_ML leaves the WDL ones
// unused), and the extra row of w2 with its bias and its output.  Again a type of its own: the three modes above keep theirs.
struct FcArgsMl : FcArgsWdl {
    const float* w2_ml;       // [n_out]: the last row of w2
    float b2_ml;
    float* moves_left;        // [n] raw output x
};
template <> struct FcArgsOf<FC_VALUE_ML> { typedef FcArgsMl T; };
template <> struct FcArgsOf<FC_WDL_ML> { typedef FcArgsMl T; };
// the moves-left sum is a fourth plane behind `red`, after the two WDL-only ones (the scalar head leaves those unused)
static_assert(4 * 256 * (int)sizeof(float) <= FC_RED_BYTES + FC_STAGE_BYTES, "the moves-left sum fits the first staging tile");

// F: features per position (180 or 360: 2 or 4 head filters x 90 squares; compile-time so that the staging loop divides
// by a constant and the K loop unrolls around a weight ring)
// exp for the running softmax statistics: v_exp_f32 (2^x) on x * log2(e) -- 2 instructions instead of libm's ~25; the
// statistics only scale the row (relative error ~1e-6 of the sum), the probabilities themselves are formed with expf in
// k_policy_normalize.  Half of this kernel's issue slots went to libm exps before (0.277 -> see profiles/r03_*).
__device__ __forceinline__ float fexp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }

// FC_WDL's finish for one position: the four waves' sums in wave order, then the softmax.  Every step treats win and loss
// alike (max(max(W, L), D), (e_W + e_L) + e_D), so that swapping the two rows of w2 / b2 negates the value and swaps the two
// probabilities bit for bit; the value is one quotient of the difference, not a difference of two rounded quotients.
template <typename A>
__device__ __forceinline__ void fc_finish_wdl(const A& a, const float* red, int bt, int ln, int board)
{
    float dw = 0.0f, dd = 0.0f, dl = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        dw += red[(bt * 4 + q) * 32 + ln];
        dd += red[256 + (bt * 4 + q) * 32 + ln];
        dl += red[512 + (bt * 4 + q) * 32 + ln];
    }
    dw += a.b2; dd += a.b2_draw; dl += a.b2_loss;
    const float mx = fmaxf(fmaxf(dw, dl), dd);
    const float ew = expf(dw - mx), ed = expf(dd - mx), el = expf(dl - mx);
    const float s = (ew + el) + ed;
    a.value[board] = (ew - el) / s;
    if (a.wdl) {
        float* o = a.wdl + (size_t)board * 3;
        o[0] = ew / s; o[1] = ed / s; o[2] = el / s;
    }
}
// (the other modes' argument type has no WDL fields: their dead branch calls this)
template <>
__device__ __forceinline__ void fc_finish_wdl<FcArgs>(const FcArgs&, const float*, int, int, int) {}

// The moves-left modes' extra running dot and its finish (the four waves' sums in wave order, like every other sum here);
// the other modes' argument types have no such row: their dead branches call the empty overloads.
__device__ __forceinline__ void fc_dot_ml(const FcArgsMl& a, float h, int j, float& dot_m) { dot_m += h * a.w2_ml[j]; }
__device__ __forceinline__ void fc_finish_ml(const FcArgsMl& a, const float* red, int bt, int ln, int board)
{
    float d = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) d += red[768 + (bt * 4 + q) * 32 + ln];
    a.moves_left[board] = d + a.b2_ml;
}
template <typename A> __device__ __forceinline__ void fc_dot_ml(const A&, float, int, float&) {}
template <typename A> __device__ __forceinline__ void fc_finish_ml(const A&, const float*, int, int, int) {}

template <int MODE, int F, typename E>
__global__ __launch_bounds__(FC_THREADS) void k_fc_tile(typename FcArgsOf<MODE>::T a, int n, const int32_t* __restrict__ n_dev)
{
    constexpr int KS = (F + 15) / 16;                 // K-steps
    constexpr int RB = KS * 32 + 16;                  // bytes per position row of the feature image; RB / 16 is odd, so
    constexpr int PART = TILE_ROWS * RB;              // the 16 lanes of a ds_read_b128 group (16 consecutive positions, same
    constexpr int RING = 6;                           // chunk) fall on 16 different 16-byte slots of the 256-byte bank row
    constexpr bool ML = MODE == FC_VALUE_ML || MODE == FC_WDL_ML;      // one more output row: moves left
    constexpr int HEAD = MODE == FC_VALUE_ML ? FC_VALUE : (MODE == FC_WDL_ML ? FC_WDL : MODE);    // the value head's own mode
    static_assert(F % 4 == 0 && KS <= FC_MAX_KSTEPS, "whole float4s per row");
    __shared__ __attribute__((aligned(16))) unsigned char lds[FC_LDS_BYTES];
    n = nn_live_boards(n, n_dev);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ln = lane & 31, kb = lane >> 5;
    const int bt = wave & 1, lq = wave >> 1;
    float* red = reinterpret_cast<float*>(lds + FC_IMG_BYTES);   // [2 values][2 position tiles][4 wave classes][32]
    unsigned char* stg = lds + FC_IMG_BYTES + FC_RED_BYTES + wave * FC_STAGE_BYTES;      // this wave's logit tile
    const int n_row_tiles = (n + TILE_ROWS - 1) / TILE_ROWS;
    struct alignas(8) Q4 { E e[4]; };
    for (int rt = blockIdx.x; rt < n_row_tiles; rt += gridDim.x) {
        const int row0 = rt * TILE_ROWS;
        // ---- stage the tile's features as (hi, lo) bf16: the tile is one contiguous block of 64 x F floats ----
        {
            const float4* src = reinterpret_cast<const float4*>(a.feat + (size_t)row0 * F);
            const int rows_here = n - row0 < TILE_ROWS ? n - row0 : TILE_ROWS;
            for (int i = tid; i < TILE_ROWS * (F / 4); i += FC_THREADS) {
                const int r = i / (F / 4), k = (i - r * (F / 4)) * 4;
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (r < rows_here) v = src[i];
                const float f[4] = {v.x, v.y, v.z, v.w};
                Q4 hi, lo;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    hi.e[j] = (E)f[j];
                    lo.e[j] = (E)(f[j] - (float)hi.e[j]);
                }
                *reinterpret_cast<Q4*>(lds + r * RB + k * 2) = hi;
                *reinterpret_cast<Q4*>(lds + PART + r * RB + k * 2) = lo;
            }
            if (KS * 16 > F) {                        // zero the K padding of the last step
                constexpr int PADQ = (KS * 16 - F) / 4;
                for (int i = tid; i < TILE_ROWS * PADQ; i += FC_THREADS) {
                    const int r = i / PADQ, k = F + (i - r * PADQ) * 4;
                    const Q4 z{};
                    *reinterpret_cast<Q4*>(lds + r * RB + k * 2) = z;
                    *reinterpret_cast<Q4*>(lds + PART + r * RB + k * 2) = z;
                }
            }
        }
        __syncthreads();

        const unsigned char* brow = lds + (bt * 32 + ln) * RB + kb * 16;
        float m_run = -3.0e38f, s_run = 0.0f;      // policy: running max / sum of exp of this lane's labels
        float dot = 0.0f;                          // value: partial hidden . w2 (WDL: the win row)
        float dot_d = 0.0f, dot_l = 0.0f;          // WDL: the draw and loss rows
        float dot_m = 0.0f;                        // moves-left modes: the extra row
        const int board = row0 + bt * 32 + ln;
        // two label tiles per pass and wave (two independent MFMA chains, one set of position operands), weights through a
        // register ring RING K-steps deep: an L2 round trip is several hundred cycles, a K-step of one tile only 96
        for (int lt0 = lq * 2; lt0 < a.n_tiles; lt0 += 8) {
            const bool two = lt0 + 1 < a.n_tiles;
            const uint4* wq0 = reinterpret_cast<const uint4*>(a.wp) + (size_t)lt0 * (KS + FC_PAD_STEPS) * 128 + lane;
            const uint4* wq1 = wq0 + (two ? (size_t)(KS + FC_PAD_STEPS) * 128 : 0);
            f32x16 acc0, acc1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
            uint4 w[RING][4];                      // [ring slot][tile 0 hi, tile 0 lo, tile 1 hi, tile 1 lo]
#pragma unroll
            for (int s = 0; s < RING - 1; ++s) {
                if (s < KS) {
                    w[s][0] = wq0[(size_t)s * 128]; w[s][1] = wq0[(size_t)s * 128 + 64];
                    w[s][2] = wq1[(size_t)s * 128]; w[s][3] = wq1[(size_t)s * 128 + 64];
                }
            }
            uint4 xh = *reinterpret_cast<const uint4*>(brow), xl = *reinterpret_cast<const uint4*>(brow + PART);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks + RING - 1 < KS) {
                    const int sl = (ks + RING - 1) % RING;
                    const size_t o = (size_t)(ks + RING - 1) * 128;
                    w[sl][0] = wq0[o]; w[sl][1] = wq0[o + 64]; w[sl][2] = wq1[o]; w[sl][3] = wq1[o + 64];
                }
                uint4 xh_n = xh, xl_n = xl;
                if (ks + 1 < KS) {
                    xh_n = *reinterpret_cast<const uint4*>(brow + (ks + 1) * 32);
                    xl_n = *reinterpret_cast<const uint4*>(brow + PART + (ks + 1) * 32);
                }
                const uint4* c = w[ks % RING];
                acc0 = FcMma<E>::mma(c[0], xh, acc0);
                acc1 = FcMma<E>::mma(c[2], xh, acc1);
                acc0 = FcMma<E>::mma(c[1], xh, acc0);
                acc1 = FcMma<E>::mma(c[3], xh, acc1);
                acc0 = FcMma<E>::mma(c[0], xl, acc0);
                acc1 = FcMma<E>::mma(c[2], xl, acc1);
                xh = xh_n; xl = xl_n;
                __builtin_amdgcn_sched_barrier(0);       // keep the loads where they are issued: RING - 1 steps ahead
            }
            // acc[4 g + i] <-> label lt * 32 + 8 g + 4 kb + i of position `board`
#pragma unroll
            for (int tile = 0; tile < 2; ++tile) {
                if (tile == 1 && !two) break;
                const int lt = lt0 + tile;
                const f32x16& acc = tile ? acc1 : acc0;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int lab = lt * 32 + g * 8 + kb * 4;
                    float v[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = lab + i < a.n_out ? acc[g * 4 + i] + a.bias[lab + i] : 0.0f;
                    if (MODE == FC_POLICY) {
                        float mx = m_run;
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (lab + i < a.n_out) mx = v[i] > mx ? v[i] : mx;
                        float s = s_run * fexp(m_run - mx);
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (lab + i < a.n_out) s += fexp(v[i] - mx);
                        m_run = mx;
                        s_run = s;
                        // into the wave's staging tile [position][32 labels]; written out in whole rows below
                        *reinterpret_cast<float4*>(stg + ln * FC_STAGE_ROW + (g * 8 + kb * 4) * 4) = make_float4(v[0], v[1], v[2], v[3]);
                    } else if (HEAD == FC_VALUE) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (lab + i < a.n_out) {
                                const float h = v[i] > 0.0f ? v[i] : 0.0f;
                                dot += h * a.w2[lab + i];
                                if (ML) fc_dot_ml(a, h, lab + i, dot_m);
                            }
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (lab + i < a.n_out) {
                                const float h = v[i] > 0.0f ? v[i] : 0.0f;
                                dot += h * a.w2[lab + i];
                                dot_d += h * a.w2[a.n_out + lab + i];
                                dot_l += h * a.w2[2 * a.n_out + lab + i];
                                if (ML) fc_dot_ml(a, h, lab + i, dot_m);
                            }
                    }
                }
                if (MODE == FC_POLICY) {
                    // the tile leaves through LDS so that HBM sees 128 contiguous bytes per position (8 lanes x 16 B) instead of
                    // 8-byte pieces from the accumulator layout (34 M write requests per launch: a request-rate limit)
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = (lane >> 3) + 8 * j, c4 = (lane & 7) * 4;
                        const float4 o = *reinterpret_cast<const float4*>(stg + r * FC_STAGE_ROW + c4 * 4);
                        const int brd = row0 + bt * 32 + r, l0 = lt * 32 + c4;
                        if (brd < n) {
                            float* dst = a.logits + (size_t)brd * a.n_out + l0;      // 8-byte aligned (n_out is even)
                            if (l0 + 3 < a.n_out) {
                                *reinterpret_cast<float2*>(dst) = make_float2(o.x, o.y);
                                *reinterpret_cast<float2*>(dst + 2) = make_float2(o.z, o.w);
                            } else {
                                if (l0 < a.n_out) dst[0] = o.x;
                                if (l0 + 1 < a.n_out) dst[1] = o.y;
                                if (l0 + 2 < a.n_out) dst[2] = o.z;
                            }
                        }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        // ---- combine: the two half-waves (kb), then the four waves that share the position tile ----
        if (MODE == FC_POLICY) {
            const float m_o = __shfl_xor(m_run, 32, 64), s_o = __shfl_xor(s_run, 32, 64);
            const float mx = m_run > m_o ? m_run : m_o;
            const float s = s_run * fexp(m_run - mx) + s_o * fexp(m_o - mx);
            if (kb == 0) {
                red[(bt * 4 + lq) * 32 + ln] = mx;
                red[256 + (bt * 4 + lq) * 32 + ln] = s;
            }
        } else {
            const float d = dot + __shfl_xor(dot, 32, 64);
            if (kb == 0) red[(bt * 4 + lq) * 32 + ln] = d;
            if (HEAD == FC_WDL) {
                const float dd = dot_d + __shfl_xor(dot_d, 32, 64), dl = dot_l + __shfl_xor(dot_l, 32, 64);
                if (kb == 0) {
                    red[256 + (bt * 4 + lq) * 32 + ln] = dd;
                    red[512 + (bt * 4 + lq) * 32 + ln] = dl;
                }
            }
            if (ML) {
                const float dm = dot_m + __shfl_xor(dot_m, 32, 64);
                if (kb == 0) red[768 + (bt * 4 + lq) * 32 + ln] = dm;
            }
        }
        __syncthreads();
        if (lq == 0 && kb == 0 && board < n) {
            if (MODE == FC_POLICY) {
                float mx = red[(bt * 4) * 32 + ln];
#pragma unroll
                for (int q = 1; q < 4; ++q) {
                    const float t = red[(bt * 4 + q) * 32 + ln];
                    mx = t > mx ? t : mx;
                }
                float s = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    s += red[256 + (bt * 4 + q) * 32 + ln] * fexp(red[(bt * 4 + q) * 32 + ln] - mx);
                a.stats[board] = make_float2(mx, s);
            } else if (HEAD == FC_VALUE) {
                float d = 0.0f;
#pragma unroll
                for (int q = 0; q < 4; ++q) d += red[(bt * 4 + q) * 32 + ln];
                a.value[board] = tanhf(d + a.b2);
            } else {
                fc_finish_wdl(a, red, bt, ln, board);
            }
            if (ML) fc_finish_ml(a, red, bt, ln, board);
        }
        __syncthreads();                    // the image and `red` are reused by the next tile
    }
}

// p = exp(logit - max) / sum, in place: one wave per row (n_out floats, n_out even: 8-byte accesses stay aligned)
__global__ __launch_bounds__(256) void k_policy_normalize(float* __restrict__ p, const float2* __restrict__ stats, int n,
                                                         int n_out, const int32_t* __restrict__ n_dev)
{
    n = nn_live_boards(n, n_dev);
    const int half = n_out / 2, lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += gridDim.x * 4) {
        const float2 st = stats[row];
        float2* r = reinterpret_cast<float2*>(p + (size_t)row * n_out);
        for (int i = lane; i < half; i += 64) {
            float2 v = r[i];
            v.x = expf(v.x - st.x) / st.y;
            v.y = expf(v.y - st.x) / st.y;
            r[i] = v;
        }
    }
}

// one dense layer's launch (dtype: the packed pairs', CZ_BF16 or CZ_F16)
template <int MODE, int F>
void launch_fc(int dtype, unsigned blocks, hipStream_t st, const typename FcArgsOf<MODE>::T& a, int n_boards, const int32_t* n_dev)
{
    if (dtype == CZ_BF16) hipLaunchKernelGGL((k_fc_tile<MODE, F, __bf16>), dim3(blocks), dim3(FC_THREADS), 0, st, a, n_boards, n_dev);
    else hipLaunchKernelGGL((k_fc_tile<MODE, F, _Float16>), dim3(blocks), dim3(FC_THREADS), 0, st, a, n_boards, n_dev);
}

}  // namespace

extern "C" size_t cz_fc_packed_elems(int n_out, int n_in)
{
    if (n_out < 1 || n_in < 1 || n_in > 2048 || n_out > 65536) return 0;
    const size_t tiles = (size_t)(n_out + 31) / 32, ksteps = (size_t)(n_in + 15) / 16;
    return tiles * (ksteps + FC_PAD_STEPS) * 2 * 64 * 8;
}

extern "C" int cz_fc_pack_weights(const float* w, int n_out, int n_in, int dtype, void* out_host)
{
    const size_t elems = cz_fc_packed_elems(n_out, n_in);
    if (!w || !out_host || elems == 0 || (dtype != CZ_BF16 && dtype != CZ_F16)) {
        czi_set_error("cz_fc_pack_weights: bad argument (dtype: CZ_BF16 or CZ_F16 pairs)");
        return CZ_ERR_ARG;
    }
    uint16_t* out = (uint16_t*)out_host;
    memset(out, 0, elems * sizeof(uint16_t));
    const int tiles = (n_out + 31) / 32, ksteps = (n_in + 15) / 16;
    for (int lt = 0; lt < tiles; ++lt)
        for (int ks = 0; ks < ksteps; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int o = lt * 32 + (lane & 31), k = ks * 16 + (lane >> 5) * 8 + j;
                    if (o >= n_out || k >= n_in) continue;
                    const float v = w[(size_t)o * n_in + k];
                    const uint16_t hi = dtype == CZ_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
                    const size_t base = (((size_t)lt * (ksteps + FC_PAD_STEPS) + ks) * 2) * 64 * 8;
                    out[base + (size_t)lane * 8 + j] = hi;
                    out[base + 64 * 8 + (size_t)lane * 8 + j] =
                        dtype == CZ_BF16 ? f32_to_bf16_bits(v - bf16_bits_to_f32(hi)) : f32_to_f16_bits(v - f16_bits_to_f32(hi));
                }
    return CZ_OK;
}

// the policy half of the tail: the logits' launch and, with `normalize`, the softmax pass
static void launch_policy_half(const float* policy_feat, int n_policy_feat, const void* wp_packed, const float* bias_p,
                               int n_labels, float* policy, float* stats_scratch, int n_boards, int dtype, int normalize,
                               const int32_t* n_dev, int n_cu, unsigned blocks, hipStream_t st)
{
    FcArgs a{};
    a.feat = policy_feat; a.wp = wp_packed; a.bias = bias_p; a.F = n_policy_feat;
    a.ksteps = (n_policy_feat + 15) / 16; a.n_out = n_labels; a.n_tiles = (n_labels + 31) / 32;
    a.logits = policy; a.stats = reinterpret_cast<float2*>(stats_scratch);
    if (n_policy_feat == 360) launch_fc<FC_POLICY, 360>(dtype, blocks, st, a, n_boards, n_dev);
    else launch_fc<FC_POLICY, 180>(dtype, blocks, st, a, n_boards, n_dev);
    if (normalize) {              // (0: `policy` keeps the raw logits -- cz_search_policy_logits takes them as they are)
        size_t nb = ((size_t)n_boards + 3) / 4;
        if (nb > (size_t)n_cu * 16) nb = (size_t)n_cu * 16;
        hipLaunchKernelGGL(k_policy_normalize, dim3((unsigned)nb), dim3(256), 0, st, policy,
                           reinterpret_cast<const float2*>(stats_scratch), n_boards, n_labels, n_dev);
    }
}

extern "C" int cz_heads_tail(const float* policy_feat, int n_policy_feat, const void* wp_packed, const float* bias_p,
                             int n_labels, const float* value_feat, int n_value_feat, const void* w1_packed,
                             const float* bias1, int n_hidden, const float* w2, float b2, float* policy, float* value,
                             float* stats_scratch, int n_boards, int dtype, int normalize, const int32_t* n_dev, void* stream)
{
    if (!policy_feat || !wp_packed || !bias_p || !value_feat || !w1_packed || !bias1 || !w2 || !policy || !value ||
        !stats_scratch || n_boards < 0 || (dtype != CZ_BF16 && dtype != CZ_F16) || n_labels < 2 || (n_labels & 1) || n_hidden < 1 || n_policy_feat < 1 ||
        (n_policy_feat != 180 && n_policy_feat != 360) || (n_value_feat != 180 && n_value_feat != 360))
        return nn_error(CZ_ERR_ARG, "cz_heads_tail: bad argument (n_labels even; 180 or 360 features per head: 2 or 4 filters x 90 squares; "
                                    "dtype of the packed pairs: CZ_BF16 or CZ_F16)");
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_heads_tail");
    if (n_cu < 0) return CZ_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    const int row_tiles = (n_boards + TILE_ROWS - 1) / TILE_ROWS;
    const unsigned blocks = nn_grid(row_tiles, 2 * n_cu);
    launch_policy_half(policy_feat, n_policy_feat, wp_packed, bias_p, n_labels, policy, stats_scratch, n_boards, dtype, normalize,
                       n_dev, n_cu, blocks, st);
    {
        FcArgs a{};
        a.feat = value_feat; a.wp = w1_packed; a.bias = bias1; a.F = n_value_feat;
        a.ksteps = (n_value_feat + 15) / 16; a.n_out = n_hidden; a.n_tiles = (n_hidden + 31) / 32;
        a.w2 = w2; a.b2 = b2; a.value = value;
        if (n_value_feat == 180) launch_fc<FC_VALUE, 180>(dtype, blocks, st, a, n_boards, n_dev);
        else launch_fc<FC_VALUE, 360>(dtype, blocks, st, a, n_boards, n_dev);
    }
    return nn_launched("cz_heads_tail");
}

extern "C" int cz_heads_tail_wdl(const float* policy_feat, int n_policy_feat, const void* wp_packed, const float* bias_p,
                                 int n_labels, const float* value_feat, int n_value_feat, const void* w1_packed,
                                 const float* bias1, int n_hidden, const float* w2, float b2_win, float b2_draw, float b2_loss,
                                 float* policy, float* value, float* wdl, float* stats_scratch, int n_boards, int dtype,
                                 int normalize, const int32_t* n_dev, void* stream)
{
    if (!policy_feat || !wp_packed || !bias_p || !value_feat || !w1_packed || !bias1 || !w2 || !policy || !value ||
        !stats_scratch || n_boards < 0 || (dtype != CZ_BF16 && dtype != CZ_F16) || n_labels < 2 || (n_labels & 1) || n_hidden < 1 || n_policy_feat < 1 ||
        (n_policy_feat != 180 && n_policy_feat != 360) || (n_value_feat != 180 && n_value_feat != 360))
        return nn_error(CZ_ERR_ARG, "cz_heads_tail_wdl: bad argument (n_labels even; 180 or 360 features per head: 2 or 4 filters x 90 squares; "
                                    "dtype of the packed pairs: CZ_BF16 or CZ_F16; wdl may be NULL)");
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_heads_tail_wdl");
    if (n_cu < 0) return CZ_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    const int row_tiles = (n_boards + TILE_ROWS - 1) / TILE_ROWS;
    const unsigned blocks = nn_grid(row_tiles, 2 * n_cu);
    launch_policy_half(policy_feat, n_policy_feat, wp_packed, bias_p, n_labels, policy, stats_scratch, n_boards, dtype, normalize,
                       n_dev, n_cu, blocks, st);
    {
        FcArgsWdl a{};
        a.feat = value_feat; a.wp = w1_packed; a.bias = bias1; a.F = n_value_feat;
        a.ksteps = (n_value_feat + 15) / 16; a.n_out = n_hidden; a.n_tiles = (n_hidden + 31) / 32;
        a.w2 = w2; a.b2 = b2_win; a.b2_draw = b2_draw; a.b2_loss = b2_loss; a.value = value; a.wdl = wdl;
        if (n_value_feat == 180) launch_fc<FC_WDL, 180>(dtype, blocks, st, a, n_boards, n_dev);
        else launch_fc<FC_WDL, 360>(dtype, blocks, st, a, n_boards, n_dev);
    }
    return nn_launched("cz_heads_tail_wdl");
}

extern "C" int cz_heads_tail_ml(const float* policy_feat, int n_policy_feat, const void* wp_packed, const float* bias_p,
                                int n_labels, const float* value_feat, int n_value_feat, const void* w1_packed,
                                const float* bias1, int n_hidden, int value_outputs, const float* w2, const float* b2,
                                float* policy, float* value, float* wdl, float* moves_left, float* stats_scratch, int n_boards,
                                int dtype, int normalize, const int32_t* n_dev, void* stream)
{
    if (!policy_feat || !wp_packed || !bias_p || !value_feat || !w1_packed || !bias1 || !w2 || !b2 || !policy || !value ||
        !moves_left || !stats_scratch || n_boards < 0 || (dtype != CZ_BF16 && dtype != CZ_F16) || n_labels < 2 || (n_labels & 1) ||
        n_hidden < 1 || n_policy_feat < 1 || (n_policy_feat != 180 && n_policy_feat != 360) ||
        (n_value_feat != 180 && n_value_feat != 360) || (value_outputs != 1 && value_outputs != 3) || (wdl && value_outputs != 3))
        return nn_error(CZ_ERR_ARG, "cz_heads_tail_ml: bad argument (n_labels even; 180 or 360 features per head: 2 or 4 filters x 90 squares; "
                                    "dtype of the packed pairs: CZ_BF16 or CZ_F16; value_outputs 1 or 3; moves_left is required; "
                                    "wdl only with value_outputs 3, may be NULL)");
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_heads_tail_ml");
    if (n_cu < 0) return CZ_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    const int row_tiles = (n_boards + TILE_ROWS - 1) / TILE_ROWS;
    const unsigned blocks = nn_grid(row_tiles, 2 * n_cu);
    launch_policy_half(policy_feat, n_policy_feat, wp_packed, bias_p, n_labels, policy, stats_scratch, n_boards, dtype, normalize,
                       n_dev, n_cu, blocks, st);
    {
        FcArgsMl a{};
        a.feat = value_feat; a.wp = w1_packed; a.bias = bias1; a.F = n_value_feat;
        a.ksteps = (n_value_feat + 15) / 16; a.n_out = n_hidden; a.n_tiles = (n_hidden + 31) / 32;
        a.w2 = w2; a.b2 = b2[0]; a.value = value;
        a.w2_ml = w2 + (size_t)value_outputs * n_hidden; a.b2_ml = b2[value_outputs]; a.moves_left = moves_left;
        if (value_outputs == 3) {
            a.b2_draw = b2[1]; a.b2_loss = b2[2]; a.wdl = wdl;
            if (n_value_feat == 180) launch_fc<FC_WDL_ML, 180>(dtype, blocks, st, a, n_boards, n_dev);
            else launch_fc<FC_WDL_ML, 360>(dtype, blocks, st, a, n_boards, n_dev);
        } else {
            if (n_value_feat == 180) launch_fc<FC_VALUE_ML, 180>(dtype, blocks, st, a, n_boards, n_dev);
            else launch_fc<FC_VALUE_ML, 360>(dtype, blocks, st, a, n_boards, n_dev);
        }
    }
    return nn_launched("cz_heads_tail_ml");
}
