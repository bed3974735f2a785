// xq_conv_input.h -- part of xq_conv.hip's translation unit; do not compile it into a second one: the unit's device code is
// compared kernel by kernel when text moves between these headers (EXPERIMENTS.md, "the convolution unit's text in headers"), and
// the search unit's kernels changed by 0.4-1.7 % when part of that unit was compiled alone.
//
// Kernel 3: k_input_conv, the 5 x 5 input convolution on the feature planes (plane_to_f), and k_split_bias_act, which makes the
// operand pair when the input layer comes from a library convolution.
#pragma once
#include "xq_nn_common.h"
#include "xq_conv_geom.h"

namespace {

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
        // (written out, not nn_live_boards: with the early return behind the call every instantiation gains or loses a few instructions)
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

}  // namespace
