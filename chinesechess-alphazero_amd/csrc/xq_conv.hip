// xq_conv.hip -- the convolutions of the policy/value ResNet as hand-written MFMA kernels (gfx950).
//
// ONE translation unit whose device side lives in internal headers (each is part of this unit only and says so; included in this
// order, which is the order the kernels are defined in):
//   xq_conv_ip4.h       k_resblock_ip4_c8 and its launch: the four-wave pair chains; the 192-filter instantiations are this unit's
//                       (the 128-filter ones are csrc/xq_conv_ip4.hip's, which has flags of its own)
//   xq_conv_kloop.h     conv_kloop, the shared K loop (9 taps x C channels out of an LDS image, weights streamed from L2), and the
//                       image's tile_load / tile_write / zero_rows_write
//   xq_conv_single.h    k_conv3x3, kernel 1: one convolution per launch, P boards per workgroup (any supported filter count / mode);
//                       k_conv3x3_c8, the same on the c8 arithmetic
//   xq_conv_block.h     k_resblock, kernel 2: a whole residual block per launch, persistent, matrix waves + copy waves; optionally
//                       the two 1x1 head convolutions folded into the last block's store pass
//   xq_conv_plain2.h    k_tower_plain2, kernel 2p: a chain of blocks on plain 2-byte operands, a pair of boards per workgroup
//   xq_conv_block_c8.h  k_resblock_c8, kernel 2c8: the block on the c8 / c6 arithmetic (FIRST: with the fused 5x5 input layer; HEADS)
//   xq_conv_pipe.h      k_resblock_pipe, kernel 2b: the 128-filter block on operand pairs, software-pipelined over boards (FIRST: the
//                       fused input layer, whose algorithm is described there)
//   xq_conv_ip.h        k_resblock_ip, k_resblock_ip_c8, kernels 2c: the two-image blocks at 192 filters
//                       (kernel 2d, the chain of 128-filter pair blocks in one launch -- k_tower_pairs4 -- lives in csrc/xq_tower.hip)
//   xq_conv_input.h     k_input_conv, kernel 3: the 5x5 input convolution on the feature planes as the search kernel writes them;
//                       k_split_bias_act: fp32 -> operand pair (used when the input layer comes from a library convolution)
// This file: the launch layer (one function per kernel) and the entry points.  The filters' host-side packing is a unit of its own,
// csrc/xq_conv_pack.hip; xq_conv_geom.h, xq_c8_kloop.h, xq_nn_common.h and xq_nn_launch.h are shared with the other network units.
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
#include "xq_conv_kloop.h"
#include "xq_conv_single.h"
#include "xq_conv_block.h"
#include "xq_conv_plain2.h"
#include "xq_conv_block_c8.h"
#include "xq_conv_pipe.h"
#include "xq_conv_ip.h"
#include "xq_conv_input.h"

namespace {

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
