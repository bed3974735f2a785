// xq_tower.hip -- CHAINS of residual blocks of the 128-filter tower in one launch (gfx950), for every tower arithmetic.
//
// Reference: the residual tower of CChessModel.build (cchess_alphazero/agent/model.py:41-43, `for _ in range(res_layer_num):
// x = self._build_residual_block(x)`, blocks at :68-83) evaluated by the prediction thread (agent/api.py:63-64).
//
// A chain takes a PAIR of boards per workgroup through all its blocks with the activations staying in LDS, so HBM sees a board at
// the chain's entry and exit only.  A peaked-policy network (what training produces) is sent to c8 / f16x3 blocks by the
// load-time guard, so every arithmetic has its chain:
//   cz_tower        c6 / c8 blocks, all of one image format, on k_resblock_ip4_c8<128> (csrc/xq_conv_ip4.hip, czi_tower4_launch).
//                   Exit: the operand triple to HBM -- a c6 chain may end on the block that writes a c8 image (the hand-over of a
//                   c6>N tower) --, (hi, lo) fp16 pairs (the hand-over of a c8>N tower to its f16x3 blocks), or the 1 x 1 head
//                   convolutions.  (One format per chain: a whole hybrid tower in one launch ran its c8 blocks 6 % slower than
//                   one launch per block.)
//   cz_tower_pairs  (hi, lo) pair blocks (f16x3 / bf16x3) on k_tower_pairs4<E, 128>, below (czi_pairs4_launch; its 192-filter
//                   form is cz_resblock_chain's).
// Arithmetic, accumulation order and conversions are those of the one-block kernels (k_resblock_c8<.., C6>, k_resblock_c8,
// k_resblock_pipe): a chain is BIT-IDENTICAL to block-by-block launches (tests/test_gpu_c6.py, tests/test_gpu_tower.py); the
// HEADS exits sum a pixel's head dot products over four 32-channel partial sums (float32 rounding of that order, within the
// bound tests/test_gpu_tower.py asserts).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/czero.h"
#include "xq_c8_kloop.h"
#include "xq_nn_common.h"
#include "xq_nn_launch.h"

// ---- kernel: the chain of PAIR blocks on four matrix waves (round 6) -----------------------------------------------------------
// k_resblock_pipe's arithmetic (three MFMAs per product: w_hi x_hi, w_lo x_hi, w_hi x_lo in that order per K-step; epilogue 1
// relu(acc + b1) -> (hi, lo); epilogue 2 ((acc + b2) + skip_hi) + skip_lo, relu, (hi, lo)) in k_resblock_ip4_c8's shape: a
// pair of boards per workgroup with ONE image each (A = rows [0, 90), B = rows [90, 180)), four matrix waves of 512 registers, no
// copy waves -- wave w takes board w >> 1 and channel tiles 2 (w & 1), + 1, so a pixel fragment read from LDS feeds two MFMAs
// per pass.  After K loop 1 (barrier: both waves of a board have read its image) a lane moves its skip elements (hi and lo
// quads of its own channels: 96 registers) out of the image and writes the intermediate activation over them; epilogue 2 writes
// the block's result to the same bytes.  Exits: the (hi, lo) pair to HBM, or the head features from hi + lo of the result, by
// items i = (pixel i >> 2, 32-channel block i & 3): per item and head output the dot product over the block's 32 channels in
// channel order, the pixel's four items summed as (a0 + a1) + (a2 + a3), + bias, relu.  Bit-identical to block-by-block launches
// of k_resblock_pipe; the heads exit within the bound tests/test_gpu_tower.py asserts.
namespace tw4 {
constexpr int MAX_BLOCKS = 12;
}  // namespace tw4

template <int CH> struct Tp4 {                  // geometry for CH filters (128: 256-byte rows; 192: 384-byte rows, chunks swizzled in groups of 8)
    static constexpr int C = CH, RB = 2 * CH, CPR = CH / 8, NT = 3, CT = CH / 32, CTW = CT / 2, NTHR = 256, KK = CH / 16;
    static constexpr bool POW2 = (RB & (RB - 1)) == 0;
    static constexpr int SWZ = POW2 ? 15 : 7;
    static constexpr int ROW_Z = 192, PSTR = (ROW_Z + 16) * RB;
    static constexpr int BIAS_OFF = 2 * PSTR, HW_OFF = BIAS_OFF + 2 * 2 * CH * 4;
    static constexpr int LDS_BYTES = HW_OFF + (CH == 128 ? 6 * CH * 4 : 0);      // (192 filters: no room for the head filters, no heads exit)
    static constexpr int W_STEP = CT * 64, W_PART = (9 * KK + W_PAD_STEPS) * W_STEP, W_RING = CH == 128 ? 4 : 3;
    static_assert(CT == 2 * CTW && KK % W_RING == 0 && KK % 2 == 0 && LDS_BYTES <= 160 * 1024, "two waves of CTW channel tiles per board");
    // byte offset of K-step kk relative to a tap's row offset (the lane's kb ^ row bits folded in)
    static __device__ __forceinline__ int kstep(int pre, int kk) { return POW2 ? pre ^ (kk << 5) : (pre ^ ((kk & 3) << 5)) + ((kk >> 2) << 7); }
    // 16-byte chunk `chunk` of pixel row `key` of board `bd` (inside a part): the swizzle key is the board-relative row
    static __device__ __forceinline__ int choff(int bd, int key, int chunk)
    {
        return (bd * 90 + key) * RB + ((chunk & ~SWZ) << 4) + (((chunk ^ key) & SWZ) << 4);
    }
};

template <typename E, int CH>
__device__ __forceinline__ void pairs_kloop_ctw(const unsigned char* lds, int row_base, const uint4* wq, int lane, f32x16* acc)
{
    typedef Tp4<CH> G;
    constexpr int RB = G::RB, NT = G::NT, CTW = G::CTW, KK = G::KK, ROW_Z = G::ROW_Z, PSTR = G::PSTR, W_STEP = G::W_STEP,
                  W_PART = G::W_PART, W_RING = G::W_RING;
    typedef typename Mfma<E>::V8 V8;
    const int kb = lane >> 5, ln = lane & 31;
    int pre[NT], pre_n[NT];
    int qy[3], qx[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int q = t * 32 + ln;
        qy[t] = q < 90 ? q / 9 : 100;
        qx[t] = q - (q / 9) * 9;
    }
    auto tap_row = [&](int dy, int dx, int t) {
        const bool ok = (unsigned)(qy[t] + dy) < 10u && (unsigned)(qx[t] + dx) < 9u;
        const int nominal = t * 32 + ln + dy * 9 + dx;
        const int row = ok ? row_base + nominal : ROW_Z + (nominal & 15);
        return row * RB + (((kb ^ nominal) & G::SWZ) << 4);   // swizzle key = the board-relative row
    };
    V8 wf[W_RING][CTW][2];
    V8 px[2][NT][2];
#pragma unroll
    for (int p = 0; p < CTW * NT; ++p)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[p][r] = 0.0f;
    auto load_w = [&](int step, int c, int part) {
        return __builtin_bit_cast(V8, wq[(size_t)part * W_PART + (size_t)step * W_STEP + c * 64]);
    };
    auto load_px = [&](int off, int part) {
        return __builtin_bit_cast(V8, *reinterpret_cast<const c8k::u32x4*>(lds + part * PSTR + off));
    };
#pragma unroll
    for (int p = 0; p < NT; ++p) pre[p] = tap_row(-1, -1, p);
#pragma unroll
    for (int s = 0; s < W_RING - 1; ++s)
#pragma unroll
        for (int c = 0; c < CTW; ++c)
#pragma unroll
            for (int part = 0; part < 2; ++part) wf[s][c][part] = load_w(s, c, part);
#pragma unroll
    for (int part = 0; part < 2; ++part)
#pragma unroll
        for (int p = 0; p < NT; ++p) px[0][p][part] = load_px(pre[p], part);
    constexpr int NM = 3 * NT * CTW, NL = NT * 2, NW = CTW * 2;
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int tt = 0; tt < 3; ++tt) {
            const int tap = 3 * j + tt;
            const int ndy = tt < 2 ? j - 1 : (j < 2 ? j : 1), ndx = tt < 2 ? tt : -1;   // the NEXT tap (last: a valid one, unused)
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const int step = tap * KK + kk;
                const int* rows = kk + 1 < KK ? pre : pre_n;
                const int kn = (kk + 1) % KK;
#pragma unroll
                for (int i = 0; i < NM; ++i) {
                    const int pass = i / (NT * CTW), p = (i % (NT * CTW)) / CTW, c = i % CTW;
                    acc[c * NT + p] = Mfma<E>::mma(wf[kk % W_RING][c][pass == 1 ? 1 : 0], px[kk & 1][p][pass == 2 ? 1 : 0], acc[c * NT + p]);
                    if (i < NL) px[(kk + 1) & 1][i % NT][i / NT] = load_px(G::kstep(rows[i % NT], kn), i / NT);
                    if (i == NM - 1 - NW && kk < NT) pre_n[kk] = tap_row(ndy, ndx, kk);
                    if (i >= NM - NW) {
                        const int idx = i - (NM - NW);
                        wf[(kk + W_RING - 1) % W_RING][idx / 2][idx % 2] = load_w(step + W_RING - 1, idx / 2, idx % 2);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#pragma unroll
            for (int p = 0; p < NT; ++p) pre[p] = pre_n[p];
        }
    }
}

template <typename E, int CH>
__global__ __launch_bounds__(256, 1) void k_tower_pairs4(
    const E* __restrict__ xh, const E* __restrict__ xl, BlockChain<tw4::MAX_BLOCKS> ch, E* __restrict__ yh, E* __restrict__ yl, int n_boards,
    const int32_t* __restrict__ n_dev, HeadArgs hd, int heads, float* __restrict__ yf_last)
{
    typedef Tp4<CH> G;
    constexpr int C = G::C, RB = G::RB, CPR = G::CPR, NT = G::NT, CTW = G::CTW, NTHR = G::NTHR, ROW_Z = G::ROW_Z, PSTR = G::PSTR,
                  BIAS_OFF = G::BIAS_OFF, HW_OFF = G::HW_OFF;
    __shared__ __attribute__((aligned(16))) unsigned char lds[G::LDS_BYTES];
    const int NB = ch.n;
    n_boards = nn_live_boards(n_boards, n_dev);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_pairs = (n_boards + 1) / 2;
    int t = blockIdx.x;
    if (t >= n_pairs) return;
    const int stride = gridDim.x;
    typedef c8k::u32x4 u4;
    constexpr int CHUNKS = 180 * CPR, LITER = (CHUNKS + NTHR - 1) / NTHR;
    auto choff = [&](int bd, int key, int chunk) { return G::choff(bd, key, chunk); };
    auto chunk_off = [&](int i) {
        const int row = i / CPR, c = i - row * CPR;
        return choff(row >= 90 ? 1 : 0, row >= 90 ? row - 90 : row, c);
    };
    auto fill = [&](int pr) __attribute__((always_inline)) {    // HBM -> images (a missing second board: zeros)
        const int have = (n_boards - 2 * pr < 2 ? n_boards - 2 * pr : 2) * 90 * CPR;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const u4* src = reinterpret_cast<const u4*>((part ? xl : xh) + (size_t)2 * pr * 90 * C);
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
                    if (it0 + j < LITER && i < CHUNKS) *reinterpret_cast<u4*>(lds + part * PSTR + chunk_off(i)) = v[j];
                }
            }
        }
    };
    auto drain = [&](int pr) __attribute__((always_inline)) {
        const int have = (n_boards - 2 * pr < 2 ? n_boards - 2 * pr : 2) * 90 * CPR;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            u4* dst = reinterpret_cast<u4*>((part ? yl : yh) + (size_t)2 * pr * 90 * C);
#pragma unroll
            for (int it = 0; it < LITER; ++it) {
                const int i = it * NTHR + tid;
                if (i < have) dst[i] = *reinterpret_cast<const u4*>(lds + part * PSTR + chunk_off(i));
            }
        }
    };
    auto write_bias = [&](int g) {                              // biases of running block g (block g % NB) into buffer g & 1
        const int blk = g % NB;
        float* dst = reinterpret_cast<float*>(lds + BIAS_OFF) + (g & 1) * 2 * C;
        if (tid < C) {
            dst[tid] = ch.b1[blk][tid];
            dst[C + tid] = ch.b2[blk][tid];
        }
        static_assert(C <= NTHR, "one thread per channel");
    };
    for (int i = tid; i < 16 * CPR; i += NTHR) {                // the shared zero rows, both parts
        *reinterpret_cast<u4*>(lds + ROW_Z * RB + i * 16) = u4{0u, 0u, 0u, 0u};
        *reinterpret_cast<u4*>(lds + PSTR + ROW_Z * RB + i * 16) = u4{0u, 0u, 0u, 0u};
    }
    fill(t);
    write_bias(0);
    write_bias(1);
    if (C == 128 && heads)
        for (int i = tid; i < 6 * C; i += NTHR) reinterpret_cast<float*>(lds + HW_OFF)[i] = hd.w[i];

    const int kb = lane >> 5, ln = lane & 31;
    const int bd = wave >> 1, tile0 = CTW * (wave & 1);
    int g = 0;
    for (;;) {
        __syncthreads();                                        // A: the images hold pair t, the bias buffers are written
        for (int blk = 0; blk < NB; ++blk, ++g) {
            const uint4* wq1 = reinterpret_cast<const uint4*>(ch.w1[blk]) + tile0 * 64 + lane;
            const uint4* wq2 = reinterpret_cast<const uint4*>(ch.w2[blk]) + tile0 * 64 + lane;
            const float* bias1 = reinterpret_cast<const float*>(lds + BIAS_OFF) + (g & 1) * 2 * C;
            const float* bias2 = bias1 + C;
            f32x16 acc[CTW * NT];
            c8k::u32x2 skh[CTW * NT][4], skl[CTW * NT][4];      // the skip operand's (hi, lo) quads, packed
            __builtin_amdgcn_s_setprio(3);
            pairs_kloop_ctw<E, CH>(lds, bd * 90, wq1, lane, acc);
            __builtin_amdgcn_s_setprio(0);
            __syncthreads();                                    // K1: both waves of a board have read its image
            int ln2 = ln, kb2 = kb;
            asm volatile("" : "+v"(ln2), "+v"(kb2));
            // epilogue 1, in place: skip <- image, image <- relu(acc + b1) as (hi, lo)
#pragma unroll
            for (int cp = 0; cp < CTW * NT; ++cp) {
                const int c = cp / NT, p = cp % NT;
                const int q = p * 32 + ln2;
                const int key = q < 90 ? q : 89;
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    const int chn = (tile0 + c) * 32 + gg * 8 + kb2 * 4;
                    const int off = choff(bd, key, chn >> 3) + (chn & 7) * 2;
                    skh[cp][gg] = *reinterpret_cast<const c8k::u32x2*>(lds + off);
                    skl[cp][gg] = *reinterpret_cast<const c8k::u32x2*>(lds + PSTR + off);
                    const float4 bv = *reinterpret_cast<const float4*>(bias1 + chn);
                    const float vv[4] = {acc[cp][gg * 4 + 0] + bv.x, acc[cp][gg * 4 + 1] + bv.y, acc[cp][gg * 4 + 2] + bv.z,
                                         acc[cp][gg * 4 + 3] + bv.w};
                    Quad<E> hi, lo;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float r = vv[i] > 0.0f ? vv[i] : 0.0f;
                        hi.e[i] = (E)r;
                        lo.e[i] = (E)(r - (float)hi.e[i]);
                    }
                    if (q < 90) {
                        *reinterpret_cast<Quad<E>*>(lds + off) = hi;
                        *reinterpret_cast<Quad<E>*>(lds + PSTR + off) = lo;
                    }
                }
            }
            __syncthreads();                                    // B: the images hold the intermediate activation; block g's b1 is consumed
            __builtin_amdgcn_s_setprio(3);
            pairs_kloop_ctw<E, CH>(lds, bd * 90, wq2, lane, acc);
            __builtin_amdgcn_s_setprio(0);
            __syncthreads();                                    // K2
            asm volatile("" : "+v"(ln2), "+v"(kb2));
            // epilogue 2, in place: image <- relu(((acc + b2) + skip_hi) + skip_lo) as (hi, lo)
#pragma unroll
            for (int cp = 0; cp < CTW * NT; ++cp) {
                const int c = cp / NT, p = cp % NT;
                const int q = p * 32 + ln2;
                if (q < 90) {
#pragma unroll
                    for (int gg = 0; gg < 4; ++gg) {
                        const int chn = (tile0 + c) * 32 + gg * 8 + kb2 * 4;
                        const int off = choff(bd, q, chn >> 3) + (chn & 7) * 2;
                        const float4 bv = *reinterpret_cast<const float4*>(bias2 + chn);
                        const Quad<E> sh = __builtin_bit_cast(Quad<E>, skh[cp][gg]), sl = __builtin_bit_cast(Quad<E>, skl[cp][gg]);
                        float v[4] = {acc[cp][gg * 4 + 0] + bv.x, acc[cp][gg * 4 + 1] + bv.y, acc[cp][gg * 4 + 2] + bv.z,
                                      acc[cp][gg * 4 + 3] + bv.w};
                        Quad<E> hi, lo;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            v[i] += (float)sh.e[i];
                            v[i] += (float)sl.e[i];
                            v[i] = v[i] > 0.0f ? v[i] : 0.0f;
                            hi.e[i] = (E)v[i];
                            lo.e[i] = (E)(v[i] - (float)hi.e[i]);
                        }
                        if (yf_last && blk == NB - 1) {          // the tower's last block: its fp32 value for the head convolutions
                            const int board = 2 * t + bd;
                            if (board < n_boards)
                                *reinterpret_cast<float4*>(yf_last + ((size_t)board * 90 + q) * C + chn) = make_float4(v[0], v[1], v[2], v[3]);
                            continue;
                        }
                        *reinterpret_cast<Quad<E>*>(lds + off) = hi;
                        *reinterpret_cast<Quad<E>*>(lds + PSTR + off) = lo;
                    }
                }
            }
            __syncthreads();                                    // C: the block's result is in the images; its b2 is consumed
            if (NB > 1) write_bias(g + 2);                      // (into the buffer block g has just released)
        }
        if (C == 128 && heads) {
            // the head features of board 2 t + bd by its two waves, from hi + lo of the result
            const int board = 2 * t + bd;
            const float* hwl = reinterpret_cast<const float*>(lds + HW_OFF);
            struct alignas(16) E8 { E e[8]; };
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                const int i = it * 128 + (wave & 1) * 64 + lane;
                if (i >= 90 * 4) continue;
                const int qq = i >> 2, b32 = i & 3;
                float a[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int off = choff(bd, qq, b32 * 4 + k);
                    const E8 h = __builtin_bit_cast(E8, *reinterpret_cast<const u4*>(lds + off));
                    const E8 l = __builtin_bit_cast(E8, *reinterpret_cast<const u4*>(lds + PSTR + off));
#pragma unroll
                    for (int o = 0; o < 6; ++o) {
                        const float4 w0 = *reinterpret_cast<const float4*>(hwl + o * C + b32 * 32 + 8 * k);
                        const float4 w1 = *reinterpret_cast<const float4*>(hwl + o * C + b32 * 32 + 8 * k + 4);
                        const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
#pragma unroll
                        for (int jj = 0; jj < 8; ++jj) a[o] += ((float)h.e[jj] + (float)l.e[jj]) * w[jj];
                    }
                }
#pragma unroll
                for (int o = 0; o < 6; ++o) {
                    a[o] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(a[o]), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
                    a[o] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(a[o]), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
                }
                if (board >= n_boards) continue;
#pragma unroll
                for (int o = 0; o < 6; ++o)
                    if ((o & 3) == b32) {
                        float hv = a[o] + hd.b[o];
                        hv = hv > 0.0f ? hv : 0.0f;
                        if (o < hd.n_pol) hd.pol[(size_t)board * (hd.n_pol * 90) + o * 90 + qq] = hv;
                        else hd.val[(size_t)board * ((6 - hd.n_pol) * 90) + (o - hd.n_pol) * 90 + qq] = hv;
                    }
            }
        } else if (!yf_last) {
            drain(t);
        }
        t += stride;
        if (t >= n_pairs) break;
        __syncthreads();                                        // (the exit has read the images)
        fill(t);
    }
}

// the pair chains' launches (cz_tower_pairs: 128 filters; cz_resblock_chain in csrc/xq_conv.hip: 192 filters, no heads exit)
template <typename E, int CH>
static void launch_pairs4(const void* x_hi, const void* x_lo, const BlockChain<tw4::MAX_BLOCKS>& ch, void* y_hi, void* y_lo,
                          HeadArgs hd, int heads, int n_boards, int n_cu, const int32_t* n_dev, hipStream_t st, float* y_f32)
{
    hipLaunchKernelGGL((k_tower_pairs4<E, CH>), dim3(nn_grid((n_boards + 1) / 2, n_cu)), dim3(256), 0, st, (const E*)x_hi,
                       (const E*)x_lo, ch, (E*)y_hi, (E*)y_lo, n_boards, n_dev, hd, heads, y_f32);
}

extern "C" int czi_pairs4_launch(const char* name, const void* x_hi, const void* x_lo, const BlockChain<12>* ch, void* y_hi,
                                 void* y_lo, const float* head_w, const float* head_b, float* pol, float* val, int n_pol,
                                 int n_boards, int channels, int dtype, int n_cu, const int32_t* n_dev, void* stream,
                                 float* y_f32)
{
    if ((channels != 128 && channels != 192) || (head_w && channels != 128)) return CZ_ERR_ARG;
    const HeadArgs hd = head_w ? HeadArgs{head_w, head_b, pol, val, n_pol} : HeadArgs{};
    const int heads = head_w ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    if (channels == 128 && dtype == CZ_F16) launch_pairs4<_Float16, 128>(x_hi, x_lo, *ch, y_hi, y_lo, hd, heads, n_boards, n_cu, n_dev, st, y_f32);
    else if (channels == 128) launch_pairs4<__bf16, 128>(x_hi, x_lo, *ch, y_hi, y_lo, hd, heads, n_boards, n_cu, n_dev, st, y_f32);
    else if (dtype == CZ_F16) launch_pairs4<_Float16, 192>(x_hi, x_lo, *ch, y_hi, y_lo, hd, heads, n_boards, n_cu, n_dev, st, y_f32);
    else launch_pairs4<__bf16, 192>(x_hi, x_lo, *ch, y_hi, y_lo, hd, heads, n_boards, n_cu, n_dev, st, y_f32);
    return nn_launched(name);
}

// ---- entry points ---------------------------------------------------------------------------------------------------------------
constexpr int TOWER_MAX_BLOCKS = 8;     // blocks per chain of cz_tower / cz_tower_pairs (model.tower_plan splits longer towers)
static_assert(TOWER_MAX_BLOCKS <= tw4::MAX_BLOCKS, "a chain fits the kernels' block list");

// One chain of c6 / c8 blocks.  fmt_x / fmt_y: per block, CZ_IMG_C8 or CZ_IMG_C6 (NULL: all CZ_IMG_C6); exit_fmt: CZ_IMG_C8 /
// CZ_IMG_C6 / CZ_IMG_PAIR, or CZ_EXIT_HEADS.
extern "C" int cz_tower(const void* x_hi, const void* x_img, int n_blocks, const void* const* w1_packed,
                        const float* const* bias1, const void* const* w2_packed, const float* const* bias2,
                        const int* fmt_x, const int* fmt_y, int exit_fmt, void* y_hi, void* y_img, const float* head_w,
                        const float* head_b, float* policy_feat, float* value_feat, int n_policy, int n_value, int n_boards,
                        const int32_t* n_dev, void* stream)
{
    const bool heads = exit_fmt == CZ_EXIT_HEADS;
    if (n_boards < 0 || !x_hi || !x_img || !w1_packed || !w2_packed || !bias1 || !bias2 || n_blocks < 1 ||
        n_blocks > TOWER_MAX_BLOCKS || (!heads && (!y_hi || !y_img)) ||
        (heads && (!head_w || !head_b || !policy_feat || !value_feat || n_policy < 1 || n_value < 1 || n_policy + n_value != 6)) ||
        (!heads && exit_fmt != CZ_IMG_C8 && exit_fmt != CZ_IMG_C6 && exit_fmt != CZ_IMG_PAIR))
        return nn_error(CZ_ERR_ARG, "cz_tower: bad argument (1 .. 8 blocks; exit CZ_IMG_C8 / CZ_IMG_C6 / CZ_IMG_PAIR with y_hi + y_img, or "
                                    "CZ_EXIT_HEADS with n_policy + n_value == 6)");
    const int fmt0 = fmt_x ? fmt_x[0] : CZ_IMG_C6;
    BlockChain<tw4::MAX_BLOCKS> ch{};
    for (int b = 0; b < n_blocks; ++b) {            // (block by block: a block's pointers are checked before its formats)
        if (!fill_chain(ch, "cz_tower", b + 1, w1_packed, bias1, w2_packed, bias2, b)) return CZ_ERR_ARG;
        const int fx = fmt_x ? fmt_x[b] : CZ_IMG_C6, fy = fmt_y ? fmt_y[b] : CZ_IMG_C6;
        if ((fx != CZ_IMG_C8 && fx != CZ_IMG_C6) || fy != fx || fx != fmt0)
            return nn_error(CZ_ERR_ARG, "cz_tower: one image format per chain, CZ_IMG_C8 or CZ_IMG_C6 (a hybrid tower is one chain per "
                                        "arithmetic -- the exit of the first hands over; pair blocks: cz_tower_pairs)");
    }
    if (!heads && ((fmt0 == CZ_IMG_C6 && exit_fmt == CZ_IMG_PAIR) || (fmt0 == CZ_IMG_C8 && exit_fmt == CZ_IMG_C6)))
        return nn_error(CZ_ERR_ARG, "cz_tower: a c6 chain ends on a c6 or c8 image, a c8 chain on a c8 image or fp16 pairs");
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_tower");
    if (n_cu < 0) return CZ_ERR_HIP;
    return czi_tower4_launch("cz_tower", x_hi, x_img, &ch, fmt0 == CZ_IMG_C6, heads ? 3 : (exit_fmt == CZ_IMG_PAIR ? 2 : 0), y_hi,
                             y_img, head_w, head_b, policy_feat, value_feat, n_policy, n_boards, n_cu, n_dev, stream);
}

// A chain of PAIR blocks ((hi, lo) operands of dtype CZ_F16 or CZ_BF16; cz_conv3x3_pack_weights filters with parts = 2):
// n_blocks launches of cz_resblock in one (bit-identical).  head_w != NULL: the chain ends on the tower's last block and writes
// the head features instead of y.
extern "C" int cz_tower_pairs(const void* x_hi, const void* x_lo, int n_blocks, const void* const* w1_packed,
                              const float* const* bias1, const void* const* w2_packed, const float* const* bias2, void* y_hi,
                              void* y_lo, const float* head_w, const float* head_b, float* policy_feat, float* value_feat,
                              int n_policy, int n_value, int n_boards, int dtype, const int32_t* n_dev, void* stream)
{
    const bool heads = head_w != nullptr;
    if (n_boards < 0 || !x_hi || !x_lo || !w1_packed || !w2_packed || !bias1 || !bias2 || n_blocks < 1 ||
        n_blocks > TOWER_MAX_BLOCKS || (dtype != CZ_F16 && dtype != CZ_BF16) || (!heads && (!y_hi || !y_lo)) ||
        (heads && (!head_b || !policy_feat || !value_feat || n_policy < 1 || n_value < 1 || n_policy + n_value != 6)))
        return nn_error(CZ_ERR_ARG, "cz_tower_pairs: bad argument (1 .. 8 blocks of (hi, lo) f16 / bf16 operands; y_hi + y_lo, or the head "
                                    "arguments with n_policy + n_value == 6)");
    BlockChain<tw4::MAX_BLOCKS> ch{};
    if (!fill_chain(ch, "cz_tower_pairs", n_blocks, w1_packed, bias1, w2_packed, bias2)) return CZ_ERR_ARG;
    if (n_boards == 0) return CZ_OK;
    const int n_cu = nn_cu_count("cz_tower_pairs");
    if (n_cu < 0) return CZ_ERR_HIP;
    return czi_pairs4_launch("cz_tower_pairs", x_hi, x_lo, &ch, y_hi, y_lo, head_w, head_b, policy_feat, value_feat, n_policy,
                             n_boards, 128, dtype, n_cu, n_dev, stream, nullptr);
}
