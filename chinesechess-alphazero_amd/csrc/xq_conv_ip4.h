// xq_conv_ip4.h -- the four-wave pair kernel of the c8 / c6 chains (k_resblock_ip4_c8) and its launch, shared by the two
// translation units that instantiate it:
//   csrc/xq_conv_ip4.hip   the 128-filter chains <128, 0, 0> and <128, 1, 1> (cz_tower), compiled with the matrix instructions'
//                          accumulators in VALU-visible registers (build.py EXTRA_FLAGS; CZ_IP4_VGPR_FORM = 1 there)
//   csrc/xq_conv.hip       the 192-filter chains (cz_resblock_chain, cz_resblock), compiled like every other unit
// Anonymous namespace, as xq_nn_common.h: each unit instantiates what it launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xq_c8_kloop.h"
#include "xq_nn_common.h"
#include "xq_nn_launch.h"
#include "xq_conv_geom.h"

// 1 in the unit that is compiled with -mllvm -amdgpu-mfma-vgpr-form (the accumulators are the MFMAs' own destination registers
// there: ip4::mfma_settle), 0 where the compiler keeps them in AGPRs and every VALU operand has gone through v_accvgpr_read.
#ifndef CZ_IP4_VGPR_FORM
#define CZ_IP4_VGPR_FORM 0
#endif

namespace {

// ---- kernel 2c / c8 / four waves: k_resblock_ip_c8's chain on FOUR matrix waves of three channel tiles each, a pair of boards
// per workgroup (round 6) -------------------------------------------------------------------------------------------------------
// 192 filters are six channel tiles.  k_resblock_ip_c8 gives each of six matrix waves one tile: two SIMDs carry two matrix waves,
// two carry one -- the convolution takes as long as the SIMDs with two, the others idle half of it, and every wave reads every
// pixel fragment from LDS for ONE MFMA.  Here a workgroup holds two boards (A = rows [0, 90), B = rows [90, 180): the X and Y rows
// of k_resblock_ip_c8 -- its arithmetic restarts the accumulators at b2 + skip inside epilogue 1, so the intermediate activation
// can be written over a board's input IN PLACE) and has four matrix waves, one per SIMD with 512 registers: wave w takes board
// w >> 1, channel tiles 3 (w & 1) .. + 2, all three pixel tiles (c8k::kloop_ctw<3, 3>: 144 accumulators, a pixel fragment feeds
// three MFMAs).  36 (tile, pixel tile, board) units, nine per SIMD.  No copy waves: the four waves write the bias buffers and
// drain / refill the pair once per chain.  A c6 piece holds the 32 channels of ONE channel tile for a pixel and is written by
// lanes that traded pixel tiles: per channel tile a wave reads the skip elements of both tiles of a trade before it writes their
// pieces.  XF / YF as in k_resblock_ip_c8 (<0, 0> c8, <1, 1> c6, <0, 1> the tower's first c6 block; a chain runs one of them).  Per accumulator tile the same products in the same order and the same
// epilogue arithmetic as k_resblock_ip_c8: bit-identical.
constexpr int IP4_EXIT_PAIRS = 2, IP4_EXIT_HEADS = 3;
// Between the K loops (128 filters; PF below): one wave per SIMD has nothing else to run while it waits for a load, so whatever
// a phase needs from global memory is requested one phase early and consumed behind the next barrier (plain loads survive
// __syncthreads()):
//   * K loop 2's first filter fragments (c8k::kloop_ctw_issue) are requested before epilogue 1 -- on c6 the correction pieces
//     only (CZ_IP4_K2_EARLY_C6 = 2: with the fp16 fragments as well, 3, the c6 kernel has the registers now but is no faster,
//     and spills 40 bytes beside the next pair's request: EXPERIMENTS.md) --, the NEXT block's K loop 1
//     fragments (the next pair's block 0 behind the last block) before epilogue 2 / the exit;
//   * block g + 2's biases are loaded before epilogue 1 and stored to LDS behind barrier B;
//   * the exits read a step's LDS operands one step ahead of the arithmetic on them;
//   * the workgroup's next pair of boards is requested ahead of the exit (fill_request: 24 loads of 16 bytes per lane) and
//     stored to the images behind the barrier that follows it (fill_store).  The exit stands behind the block loop for
//     that: the request's 96 registers are live across the exit and the drain only.
// Per accumulator tile the products and every sum keep their order: bit-identical.  At 192 filters the kernel spills already
// and keeps the plain order (PF = 0).  CZ_IP4_PREFETCH (variant builds, tools/ip4_stamps.py): a mask of the items above
// (1 K loop 2's fragments, 16 the next K loop 1's, 4 biases, 8 exits, 32 the next pair), 0 = the plain order everywhere.
// (Requesting the next block's scale bytes and exponent words a block early as well measured 0.6 % slower: EXPERIMENTS.md.)
#ifndef CZ_IP4_PREFETCH
#define CZ_IP4_PREFETCH 61
#endif
#ifndef CZ_IP4_K2_EARLY_C6
#define CZ_IP4_K2_EARLY_C6 2
#endif
// The in-place epilogues and the staging in front of the exits run with every wave behind the same barrier and nothing
// beside them, so their time is their instruction count.  CZ_IP4_EPI (variant builds, as CZ_IP4_PREFETCH): a mask of what
// is taken out of them, each item with the same values in the same order -- bit-identical; 0 = the earlier instruction forms.
//    1  relu(acc) is ONE v_max_f32 0, x (ip4::relu1): the compiler puts a canonicalising v_max_f32 x, x in front of
//       a > 0 ? a : 0, which only alters signalling NaNs, and MFMA / v_pk_add_f32 results hold none;
//    2  the fp16 halves of a quad are converted two at a time (v_cvt_pk_f16_f32, round to nearest even: ip4::Half4);
//    4  (128 filters) an epilogue computes a swizzled row base per pixel tile -- the f16 row with the key and the lane's
//       half chunk folded in, the piece row -- and forms every access with one xor of a compile-time chunk;
//    8  (with 4) the padding lanes of pixel tile 2 (pixels 90 .. 95) get a dump row behind the head filters as their base
//       instead of exec masking around every store;
//   16  (with 4, c6) pixel tile 2 of BOTH channel tiles of a wave is one unit: the trade leaves tile0's 32 channels of pixel
//       64 + ln in the lower lanes and tile0 + 1's in the upper ones, every lane stores a piece (self-paired, each unit
//       made every piece twice).  Epilogue 1 reads the skip elements of both tiles before that unit writes;
#ifndef CZ_IP4_EPI
#define CZ_IP4_EPI 31
#endif
namespace ip4 {
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
// (The asm is opaque to the compiler's MFMA -> VALU hazard recogniser, which pads nothing in front of it: `a` must not be
// read out of an MFMA's destination registers before that MFMA has written them.  Where the accumulators sit in AGPRs every
// operand has gone through v_accvgpr_read or v_pk_add_f32, which the compiler pads; where they are the MFMAs' own VGPRs
// (CZ_IP4_VGPR_FORM) the kernel puts ip4::mfma_settle behind each K loop, ahead of every reader.)
template <bool ONE> __device__ __forceinline__ float relu1(float a)
{
    if (ONE) {
        float r;
        asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(a));
        return r;
    }
    return a > 0.0f ? a : 0.0f;
}
// Behind a K loop, ahead of the first reader of an accumulator, where the accumulators are the MFMAs' destination VGPRs: the
// wait states of the ISA's "XDL write VGPR -> VALU read" rule for the longest MFMA of the loops.  On gfx950 that is passes + 4
// (LLVM's GCNHazardRecognizer: passes + 3, one more on gfx950 above two passes): 20 for the 16-pass
// v_mfma_scale_f32_32x32x64_f8f6f4 on e4m3 operands, 12 for its 8-pass bf6 form and for v_mfma_f32_32x32x16_f16 -- s_nop 15 +
// s_nop 3 is also what the compiler itself puts between such an MFMA and a v_max_f32 of its result.  The tiles are "+v"
// operands: every later reader of an accumulator depends on this statement, so none can be scheduled above it.
template <int N> __device__ __forceinline__ void mfma_settle(f32x16* acc)
{
    static_assert(N == 6 || N == 9, "a wave's accumulator tiles: 2 or 3 channel tiles x 3 pixel tiles");
    if constexpr (N == 6)
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]));
    else
        asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]),
                                             "+v"(acc[6]), "+v"(acc[7]), "+v"(acc[8]));
}
// four fp32 values -> their fp16 quad (the 8 bytes of a Quad<_Float16>), and the quad's values back
struct Half4 {
    f16x2 a, b;
    template <bool PK> __device__ __forceinline__ void set(const float* r)
    {
        if (PK) {
            a = __builtin_convertvector(f32x2{r[0], r[1]}, f16x2);
            b = __builtin_convertvector(f32x2{r[2], r[3]}, f16x2);
        } else {
            a[0] = (_Float16)r[0]; a[1] = (_Float16)r[1];
            b[0] = (_Float16)r[2]; b[1] = (_Float16)r[3];
        }
    }
    __device__ __forceinline__ float get(int i) const { return (float)(i < 2 ? a[i] : b[i - 2]); }
    __device__ __forceinline__ c8k::u32x2 bits() const
    {
        return c8k::u32x2{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b)};
    }
};
}  // namespace ip4
#ifdef CZ_IP4_STAMPS
// timing build (tools/ip4_stamps.py; never the default library): shader-cycle stamps of one wave per board around the phases
// of every block of workgroup 0's second pair -- [board][block][IP4_STAMP_*]
__device__ long long g_ip4_stamps[2 * 12 * 16];
#define IP4_STAMP(i) do { if (stamp_on) g_ip4_stamps[(bd * 12 + blk) * 16 + (i)] = clock64(); } while (0)
struct Ip4FirstMfma {
    long long* at;
    __device__ __forceinline__ void first_mfma() { if (at) *at = clock64(); }
};
#define IP4_HOOK(i) Ip4FirstMfma{stamp_on ? &g_ip4_stamps[(bd * 12 + blk) * 16 + (i)] : nullptr}
// (the whole K loop, with the stamp behind its first MFMA)
#define IP4_KLOOP(FMT, flt, sxl, sx, i) do { c8k::CtwFrags<CTW> st_; \
        c8k::kloop_ctw_run<CTW, NT, C, FMT, Ip4FirstMfma, 3>(lds, img, flt, st_, lane, acc, sxl, sx, IP4_HOOK(i)); } while (0)
#else
#define IP4_KLOOP(FMT, flt, sxl, sx, i) c8k::kloop_ctw<CTW, NT, C, FMT>(lds, img, flt, lane, acc, sxl, sx)
#define IP4_STAMP(i) do { } while (0)
#define IP4_HOOK(i) c8k::NoHook()
#endif
// MIX (with <1, 1>): the chain starts the tower -- its block 0 reads the input layer's c8 image (first filter c8-packed: CZ_F16C86)
template <int C, int XF, int YF, bool MIX = false>
__global__ __launch_bounds__(256, 1) void k_resblock_ip4_c8(
    const _Float16* __restrict__ xh, const unsigned char* __restrict__ xc, BlockChain<ip::MAX_BLOCKS> ch, _Float16* __restrict__ yh,
    unsigned char* __restrict__ yc, float* __restrict__ yf_last, int n_boards, const int32_t* __restrict__ n_dev,
    int exit_mode, HeadArgs hd)
{
    typedef Geom<C, 1, 2> G;
    constexpr int RB = G::RB, CPR = G::CPR, NT = 3, CTW = G::CT / 2, NTHR = 256;
    static_assert(G::CT == 2 * CTW, "two waves of CTW channel tiles per board");
    constexpr int PSTR = ip::ROWS * RB;                         // bytes per operand part
    constexpr int BIAS_OFF = 2 * PSTR;
    constexpr int CHUNKS = 180 * CPR, LITER = (CHUNKS + NTHR - 1) / NTHR;
    // exit_mode (the chain's LAST block, 128 filters: cz_tower's exits): 0 = the operand pair / fp32 (yf_last); IP4_EXIT_PAIRS =
    // (hi, lo) fp16 pairs [n][90][C] to yh and yc; IP4_EXIT_HEADS = the six 1 x 1 head features (hd).  Both stage relu(acc) as fp32
    // in the board's dead image ([pixel][64 channels] per part, 16-byte chunks swizzled by the pixel); the board's two waves then
    // take items i = (pixel i >> 2, 32-channel block i & 3).  PAIRS: hi = fp16(r), lo = fp16(r - hi) per value, bit-identical to
    // block-by-block launches.  HEADS: per item and head output the dot product over the block's 32 channels in channel order,
    // the pixel's four items summed as (a0 + a1) + (a2 + a3), + bias, relu -- within the bound tests/test_gpu_tower.py asserts
    // against the one-block HEADS kernels (their sums associate differently).
    constexpr int HW_OFF = BIAS_OFF + 2 * 2 * C * 4;
    constexpr int DUMP_OFF = HW_OFF + 6 * C * 4;                // (128 filters) one row for the stores of padding lanes
    static_assert(C != 128 || DUMP_OFF % RB == 0, "the dump row is swizzled like an image row");
    __shared__ __attribute__((aligned(16))) unsigned char lds[HW_OFF + (C == 128 ? 6 * C * 4 + RB : 0)];   // bias[2 buffers][2 convolutions][C] | head filters | dump row
    // what is taken out of the epilogues (the mask above the kernel).  The c6 chain that starts a 192-filter tower keeps the
    // code before: with items 1 and 2 its scratch grows (276 -> 444 bytes per lane)
    constexpr int EP = MIX ? 0 : (CZ_IP4_EPI);
    constexpr bool EADR = C == 128 && (EP & 4) != 0;            // row bases per epilogue
    constexpr bool EDMP = EADR && (EP & 8) != 0;                // padding lanes store to the dump row
    constexpr bool EC6U = EADR && XF == 1 && YF == 1 && !MIX;   // the c6 units on row bases
    constexpr bool EMRG = EC6U && (EP & 16) != 0;               // tile 2 of both channel tiles in one unit
    const int NB = ch.n;
    n_boards = nn_live_boards(n_boards, n_dev);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_pairs = (n_boards + 1) / 2;
    int t = blockIdx.x;
    if (t >= n_pairs) return;
    const int stride = gridDim.x;
    typedef c8k::u32x4 u4;
    // 16-byte chunk `chunk` of pixel row `key` of board `bd` (inside a part): the swizzle key is the board-relative row
    auto choff = [&](int bd, int key, int chunk) {
        return (bd * 90 + key) * RB + ((chunk & ~G::SWZ) << 4) + (((chunk ^ key) & G::SWZ) << 4);
    };
    auto chunk_off = [&](int i) {                               // chunk i of the pair
        const int row = i / CPR, c = i - row * CPR;
        return choff(row >= 90 ? 1 : 0, row >= 90 ? row - 90 : row, c);
    };
    auto fill = [&](int pr) __attribute__((always_inline)) {    // HBM -> images (a missing second board: zeros)
        const int have = (n_boards - 2 * pr < 2 ? n_boards - 2 * pr : 2) * 90 * CPR;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const u4* src = part ? reinterpret_cast<const u4*>(xc + (size_t)2 * pr * 90 * 2 * C)
                                 : reinterpret_cast<const u4*>(xh + (size_t)2 * pr * 90 * C);
#pragma unroll
            for (int it0 = 0; it0 < LITER; it0 += 9) {
                u4 v[9];
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    const int i = (it0 + j) * NTHR + tid;
                    v[j] = u4{0u, 0u, 0u, 0u};
                    if (it0 + j < LITER && i < have) v[j] = src[i];
                }
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    const int i = (it0 + j) * NTHR + tid;
                    if (it0 + j < LITER && i < CHUNKS) *reinterpret_cast<u4*>(lds + part * PSTR + chunk_off(i)) = v[j];
                }
            }
        }
    };
    // fill in two halves (PF & 32): pair pr's chunks requested into registers, and stored to the images once nobody reads them
    auto fill_request = [&](int pr, u4 (&v)[2][LITER]) __attribute__((always_inline)) {
        const int have = (n_boards - 2 * pr < 2 ? n_boards - 2 * pr : 2) * 90 * CPR;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            const u4* src = part ? reinterpret_cast<const u4*>(xc + (size_t)2 * pr * 90 * 2 * C)
                                 : reinterpret_cast<const u4*>(xh + (size_t)2 * pr * 90 * C);
#pragma unroll
            for (int it = 0; it < LITER; ++it) {
                const int i = it * NTHR + tid;
                v[part][it] = u4{0u, 0u, 0u, 0u};
                if (i < have) v[part][it] = src[i];
            }
        }
    };
    auto fill_store = [&](const u4 (&v)[2][LITER]) __attribute__((always_inline)) {
#pragma unroll
        for (int part = 0; part < 2; ++part)
#pragma unroll
            for (int it = 0; it < LITER; ++it) {
                const int i = it * NTHR + tid;
                if (i < CHUNKS) *reinterpret_cast<u4*>(lds + part * PSTR + chunk_off(i)) = v[part][it];
            }
    };
    auto drain = [&](int pr) __attribute__((always_inline)) {
        const int have = (n_boards - 2 * pr < 2 ? n_boards - 2 * pr : 2) * 90 * CPR;
#pragma unroll
        for (int part = 0; part < 2; ++part) {
            u4* dst = part ? reinterpret_cast<u4*>(yc + (size_t)2 * pr * 90 * 2 * C) : reinterpret_cast<u4*>(yh + (size_t)2 * pr * 90 * C);
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
        for (int i = tid; i < C; i += NTHR) {
            dst[i] = ch.b1[blk][i];
            dst[C + i] = ch.b2[blk][i];
        }
    };
    for (int i = tid; i < 16 * CPR; i += NTHR) {                // the shared zero rows, both parts
        *reinterpret_cast<u4*>(lds + ip::ROW_Z * RB + i * 16) = u4{0u, 0u, 0u, 0u};
        *reinterpret_cast<u4*>(lds + PSTR + ip::ROW_Z * RB + i * 16) = u4{0u, 0u, 0u, 0u};
    }
    fill(t);
    write_bias(0);
    write_bias(1);
    if (C == 128 && exit_mode == IP4_EXIT_HEADS)
        for (int i = tid; i < 6 * C; i += NTHR) reinterpret_cast<float*>(lds + HW_OFF)[i] = hd.w[i];

    const int kb = lane >> 5, ln = lane & 31;
    const int bd = wave >> 1, tile0 = CTW * (wave & 1);         // this wave's board and first channel tile
    // this lane's four channels chn .. chn + 3 of pixel row `key` of its board: the f16 quad, its lo8 word, its e4m3(x) word
    auto offs = [&](int key, int chn, int& off, int& off_lo, int& off_hi) {
        off = choff(bd, key, chn >> 3) + (chn & 7) * 2;
        off_lo = PSTR + choff(bd, key, chn >> 4) + (chn & 15);
        off_hi = PSTR + choff(bd, key, CPR / 2 + (chn >> 4)) + (chn & 15);
    };
    // byte offset of channels chn .. chn + 3 (fp32) of pixel q in the board's staging (128 filters)
    auto stg = [&](int q, int chn) {
        return (chn >> 6) * PSTR + (bd * 90 + q) * RB + (((((chn & 63) >> 2)) ^ (q & 15)) << 4);
    };
    // one unit of a c6 image: channel tile tc, pixel tiles (0, 1) (pp = 0) or tile 2 with itself (pp = 1) of this wave's board.
    // relu(a*) -> f16 quads + the two bf6 pieces of a pixel's 32 channels (exponent k); a* keep relu(a*).
    auto write_c6_unit = [&](f32x16& aa, f32x16& ab, int tc, int pp, int k, int ln2, int kb2) __attribute__((always_inline)) {
        using rb8::u32x6;
        const float s_hi = __builtin_ldexpf(1.0f, k), s_lo = __builtin_ldexpf(1.0f, k - cf8::X_LO_SHIFT);
        f32x16 lo_a, lo_b;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && pp == 1) break;
            const int tt = pp == 0 ? h : 2;
            const int q = tt * 32 + ln2;
            const int key = q < 90 ? q : 89;
            f32x16& a = h ? ab : aa;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const int chn = tc * 32 + gg * 8 + kb2 * 4;
                float r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = ip4::relu1<(EP & 1) != 0>(a[gg * 4 + i]);
                ip4::Half4 hq;
                hq.template set<(EP & 2) != 0>(r);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[gg * 4 + i] = r[i];
                    (h ? lo_b : lo_a)[gg * 4 + i] = r[i] - hq.get(i);
                }
                if (q < 90) *reinterpret_cast<c8k::u32x2*>(lds + choff(bd, key, chn >> 3) + (chn & 7) * 2) = hq.bits();
            }
        }
        if (pp == 1) lo_b = lo_a;
        f32x16 av, bv, al, bl;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const auto sv = __builtin_amdgcn_permlane32_swap(__float_as_uint(aa[r]), __float_as_uint(pp == 0 ? ab[r] : aa[r]), false, false);
            const auto sl = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo_a[r]), __float_as_uint(lo_b[r]), false, false);
            av[r] = __uint_as_float(sv[0]); bv[r] = __uint_as_float(sv[1]);
            al[r] = __uint_as_float(sl[0]); bl[r] = __uint_as_float(sl[1]);
        }
        const u32x6 pl = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(al, bl, s_lo);
        const u32x6 pv = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(av, bv, s_hi);
        const int q = pp == 0 ? kb2 * 32 + ln2 : 64 + ln2;
        if (pp == 0 || (kb2 == 0 && q < 90)) {
            const int c0 = 4 * (tc >> 1) + 2 * (tc & 1), c1 = CPR / 2 + c0;
            unsigned char* P1 = lds + PSTR;
            *reinterpret_cast<u4*>(P1 + choff(bd, q, c0)) = u4{pl[0], pl[1], pl[2], pl[3]};
            *reinterpret_cast<c8k::u32x2*>(P1 + choff(bd, q, c0 + 1)) = c8k::u32x2{pl[4], pl[5]};
            *reinterpret_cast<u4*>(P1 + choff(bd, q, c1)) = u4{pv[0], pv[1], pv[2], pv[3]};
            *reinterpret_cast<c8k::u32x2*>(P1 + choff(bd, q, c1 + 1)) = c8k::u32x2{pv[4], pv[5]};
        }
    };
    // ---- the epilogues on row bases (EADR; 128 filters: RB = 256, the swizzle covers the row's 16 chunks) ----
    // An access of pixel q, chunk ck is row(q) * RB + ((ck ^ q) & 15) * 16 + const: with base = row(q) * RB + ((q & 15) ^ ck0) * 16
    // + const it is base ^ (ck1 << 4) for any split ck = ck0 ^ ck1 -- ck0 takes the wave's first channel tile and the lane's
    // half, ck1 is known at compile time.  EDMP: a padding lane's base is its own 16-byte slot of the dump row (the xor keeps
    // it inside the row), so it reads rubbish for pixels nobody stores and writes where nobody reads.
    struct EpiBases {
        int h[3];               // pixel tile tt, f16 row: this lane's quad of chunk 4 tile0 (^ 4 c + gg)
        int p[3];               // pixel tile tt, piece row (part 1): chunk 2 tile0 (^ 2 c + j, ^ 8 for the value piece)
        int s[3];               // pixel tile tt, fp32 staging row: chunk kb (^ 8 c + 2 gg)
        int pw01;               // the piece this lane writes after a trade of tiles (0, 1): pixel 32 kb + ln
        int dump;
        bool ok2;               // pixel 64 + ln exists
    };
    auto epi_bases = [&](EpiBases& e, int ln2, int kb2, bool pieces, bool staging) __attribute__((always_inline)) {
        e.ok2 = 64 + ln2 < 90;
        e.dump = DUMP_OFF + ((ln2 - 26) * 2 + kb2) * 16;
#pragma unroll
        for (int tt = 0; tt < 3; ++tt) {
            const int q = tt * 32 + ln2;
            const int key = tt < 2 || e.ok2 ? q : 89;           // (without the dump row a padding lane reads row 89)
            const int row = (bd * 90 + key) * RB;
            const bool dmp = EDMP && tt == 2;
            if (!staging) e.h[tt] = dmp && !e.ok2 ? e.dump : row + (((key & 15) ^ (4 * tile0)) << 4) + kb2 * 8;
            if (pieces) e.p[tt] = dmp && !e.ok2 ? e.dump : PSTR + row + (((key & 15) ^ (2 * tile0)) << 4);
            if (staging) e.s[tt] = dmp && !e.ok2 ? e.dump : (tile0 >> 1) * PSTR + row + (((key & 15) ^ kb2) << 4);
        }
        if (pieces) {
            const int q = kb2 * 32 + ln2;
            e.pw01 = PSTR + (bd * 90 + q) * RB + (((q & 15) ^ (2 * tile0)) << 4);
        }
    };
    // write_c6_unit on row bases.  pp = 0: pixel tiles (0, 1) of relative channel tile c; pp = 1: tile 2 of c with itself; pp = 2
    // (EMRG): aa / ab = tile 2 of relative channel tiles 0 / 1 -- the lower lanes leave the trade with tile0's 32 channels
    // of pixel 64 + ln, the upper lanes with tile0 + 1's, and both store their piece.
    auto c6_unit = [&](f32x16& aa, f32x16& ab, int pp, int c, int k, const EpiBases& e, int kb2) __attribute__((always_inline)) {
        using rb8::u32x6;
        const float s_hi = __builtin_ldexpf(1.0f, k), s_lo = __builtin_ldexpf(1.0f, k - cf8::X_LO_SHIFT);
        f32x16 lo_a, lo_b;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h == 1 && pp == 1) break;
            const int tt = pp == 0 ? h : 2;
            const int x = pp == 2 ? h : c;
            f32x16& a = h ? ab : aa;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                float r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = ip4::relu1<(EP & 1) != 0>(a[gg * 4 + i]);
                ip4::Half4 hq;
                hq.template set<(EP & 2) != 0>(r);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[gg * 4 + i] = r[i];
                    (h ? lo_b : lo_a)[gg * 4 + i] = r[i] - hq.get(i);
                }
                if (EDMP || tt < 2 || e.ok2) *reinterpret_cast<c8k::u32x2*>(lds + (e.h[tt] ^ ((4 * x + gg) << 4))) = hq.bits();
            }
        }
        if (pp == 1) lo_b = lo_a;
        f32x16 av, bv, al, bl;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const auto sv = __builtin_amdgcn_permlane32_swap(__float_as_uint(aa[r]), __float_as_uint(pp == 1 ? aa[r] : ab[r]), false, false);
            const auto sl = __builtin_amdgcn_permlane32_swap(__float_as_uint(lo_a[r]), __float_as_uint(lo_b[r]), false, false);
            av[r] = __uint_as_float(sv[0]); bv[r] = __uint_as_float(sv[1]);
            al[r] = __uint_as_float(sl[0]); bl[r] = __uint_as_float(sl[1]);
        }
        const u32x6 pl = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(al, bl, s_lo);
        const u32x6 pv = __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(av, bv, s_hi);
        // the piece row of the pixel this lane holds, and the chunk of its channel tile that the base does not carry
        const bool pok = pp == 0 || (e.ok2 && (pp == 2 || kb2 == 0));
        int pw = pp == 0 ? e.pw01 : pp == 2 ? e.p[2] ^ (kb2 << 5) : e.p[2];
        if (EDMP && pp == 1) pw = kb2 == 0 ? pw : e.dump;
        const int pc = pp == 2 ? 0 : 2 * c;
        if (EDMP || pok) {
            *reinterpret_cast<u4*>(lds + (pw ^ (pc << 4))) = u4{pl[0], pl[1], pl[2], pl[3]};
            *reinterpret_cast<c8k::u32x2*>(lds + (pw ^ ((pc + 1) << 4))) = c8k::u32x2{pl[4], pl[5]};
            *reinterpret_cast<u4*>(lds + (pw ^ ((8 + pc) << 4))) = u4{pv[0], pv[1], pv[2], pv[3]};
            *reinterpret_cast<c8k::u32x2*>(lds + (pw ^ ((9 + pc) << 4))) = c8k::u32x2{pv[4], pv[5]};
        }
    };
    // (epilogue 1) b2 + this lane's skip elements of pixel tile tt, relative channel tile c, out of a c6 image
    auto c6_skip = [&](f32x16& sk, int tt, int c, int k_x, const float* bias2, const EpiBases& e, int kb2) __attribute__((always_inline)) {
        const u4 hd4 = *reinterpret_cast<const u4*>(lds + (e.p[tt] ^ ((2 * c) << 4)));
        const c8k::u32x2 tl2 = *reinterpret_cast<const c8k::u32x2*>(lds + (e.p[tt] ^ ((2 * c + 1) << 4)));
        const uint32_t wv[7] = {hd4.x, hd4.y, hd4.z, hd4.w, tl2.x, tl2.y, 0u};
        const uint32_t sh6 = (uint32_t)kb2 * 6u;
        rb8::u32x6 pc;
#pragma unroll
        for (int w = 0; w < 6; ++w) pc[w] = __builtin_amdgcn_alignbit(wv[w + 1], wv[w], sh6);
        const rb8::f32x32 xl = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(pc, __builtin_ldexpf(1.0f, k_x - cf8::X_LO_SHIFT));
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {
            const int chn = (tile0 + c) * 32 + gg * 8 + kb2 * 4;
            const float4 bv = *reinterpret_cast<const float4*>(bias2 + chn);
            float vv[4] = {bv.x, bv.y, bv.z, bv.w};
            const Quad<_Float16> xq = *reinterpret_cast<const Quad<_Float16>*>(lds + (e.h[tt] ^ ((4 * c + gg) << 4)));
#pragma unroll
            for (int i = 0; i < 4; ++i) vv[i] += (float)xq.e[i] + xl[2 * (gg * 4 + i)];
#pragma unroll
            for (int i = 0; i < 4; ++i) sk[gg * 4 + i] = vv[i];
        }
    };
    constexpr int PF = C == 128 ? (CZ_IP4_PREFETCH) : 0;        // what is requested a phase early (the mask above the kernel)
    constexpr bool FE = (PF & 32) != 0;                         // the next pair's images requested ahead of the exit
    constexpr int K2E = YF ? (CZ_IP4_K2_EARLY_C6) : 3;          // the parts of K loop 2's fragments requested before epilogue 1
    static_assert(!MIX || PF == 0, "the early requests assume one image format per chain");
    static_assert(C <= NTHR, "a thread carries one bias of each convolution");
    // the first fragments of block blk's K loop 1 (they depend on the filter alone)
    c8k::CtwFrags<CTW> frags;
    auto issue_k1 = [&](int blk) __attribute__((always_inline)) {
        c8k::Filter f[CTW];
#pragma unroll
        for (int c = 0; c < CTW; ++c) f[c] = c8k::make_filter<C>(ch.w1[blk], tile0 + c, lane, 0, 0);
        c8k::kloop_ctw_issue<CTW, C, XF>(f, frags);
    };
    if (PF & 16) issue_k1(0);
#ifdef CZ_IP4_STAMPS
    int pair_no = 0;
#endif
    int g = 0;                                                  // running block count: its parity picks the bias buffer
    for (;;) {
        __syncthreads();                                        // A: the images hold pair t, the bias buffers are written
#ifdef CZ_IP4_STAMPS
        const bool stamp_on = blockIdx.x == 0 && (wave & 1) == 0 && pair_no == 1;
        ++pair_no;
#endif
        for (int blk = 0; blk < NB; ++blk, ++g) {
            IP4_STAMP(0);
            const void* w1p = ch.w1[blk];
            const void* w2p = ch.w2[blk];
            const int blk_next = blk + 1 == NB ? 0 : blk + 1;
            static_assert(!MIX || (XF == 1 && YF == 1), "a c6 chain whose first block reads a c8 image");
            const bool xf = MIX ? blk != 0 : XF != 0;           // the format of the image this block's first convolution reads
            c8k::Filter flt1[CTW], flt2[CTW];
#pragma unroll
            for (int c = 0; c < CTW; ++c) {
                flt1[c] = c8k::make_filter<C>(w1p, tile0 + c, lane);
                flt2[c] = c8k::make_filter<C>(w2p, tile0 + c, lane);
            }
            const int* ints1 = reinterpret_cast<const int*>(reinterpret_cast<const uint4*>(w1p) + c8k::Geo<C>::MAIN_U4 + c8k::Geo<C>::C8_U4);
            const int* ints2 = reinterpret_cast<const int*>(reinterpret_cast<const uint4*>(w2p) + c8k::Geo<C>::MAIN_U4 + c8k::Geo<C>::C8_U4);
            const int k_x = xf ? __builtin_amdgcn_readfirstlane(ints1[2]) : 0;
            const int k_y = YF ? __builtin_amdgcn_readfirstlane(ints2[2]) : 0;
            const int k_out = YF ? __builtin_amdgcn_readfirstlane(ints2[3]) : CZ_C6_OUT_C8;
            const float* bias1 = reinterpret_cast<const float*>(lds + BIAS_OFF) + (g & 1) * 2 * C;
            const float* bias2 = bias1 + C;
            float* yf = blk == NB - 1 ? yf_last : nullptr;      // fp32 output: the chain's last block only
            f32x16 acc[CTW * NT];
#pragma unroll
            for (int c = 0; c < CTW; ++c)
#pragma unroll
                for (int gg = 0; gg < 4; ++gg) {
                    const float4 bv = *reinterpret_cast<const float4*>(bias1 + (tile0 + c) * 32 + gg * 8 + kb * 4);
#pragma unroll
                    for (int p = 0; p < NT; ++p) {
                        acc[c * NT + p][gg * 4 + 0] = bv.x; acc[c * NT + p][gg * 4 + 1] = bv.y;
                        acc[c * NT + p][gg * 4 + 2] = bv.z; acc[c * NT + p][gg * 4 + 3] = bv.w;
                    }
                }
            const c8k::Image img{bd * 90, ip::ROW_Z, PSTR};
            __builtin_amdgcn_s_setprio(3);
            IP4_STAMP(1);
            if (MIX && !xf) IP4_KLOOP(0, flt1, 127 - cf8::X_LO_SHIFT, 127, 2);
            else if (!(PF & 16)) IP4_KLOOP(XF, flt1, 127 + k_x - cf8::X_LO_SHIFT, 127 + k_x, 2);
            else c8k::kloop_ctw_run<CTW, NT, C, XF>(lds, img, flt1, frags, lane, acc, 127 + k_x - cf8::X_LO_SHIFT, 127 + k_x, IP4_HOOK(2));
            if (CZ_IP4_VGPR_FORM) ip4::mfma_settle<CTW * NT>(acc);
            __builtin_amdgcn_s_setprio(0);
            IP4_STAMP(3);
            __syncthreads();                                    // K1: both waves of a board have read its image
            IP4_STAMP(4);
            int ln2 = ln, kb2 = kb;
            asm volatile("" : "+v"(ln2), "+v"(kb2));
            // in flight under epilogue 1: K loop 2's first fragments, block g + 2's biases
            if (PF & 1) c8k::kloop_ctw_issue<CTW, C, YF, K2E>(flt2, frags);
            float nb1 = 0.0f, nb2 = 0.0f;
            if ((PF & 4) && NB > 1 && tid < C) {
                nb1 = ch.b1[(g + 2) % NB][tid];
                nb2 = ch.b2[(g + 2) % NB][tid];
            }
            // epilogue 1, in place: this lane's skip elements out of the image, relu(acc) in the operand format over them, the
            // freed accumulators restart at b2 + skip
            EpiBases eb;
            if (EC6U) epi_bases(eb, ln2, kb2, true, false);
#pragma unroll
            for (int c = 0; c < CTW; ++c) {
                const int tc = tile0 + c;
                if (EC6U) {
                    f32x16 sk[2];
                    c6_skip(sk[0], 0, c, k_x, bias2, eb, kb2);
                    c6_skip(sk[1], 1, c, k_x, bias2, eb, kb2);
                    c6_unit(acc[c * NT + 0], acc[c * NT + 1], 0, c, k_y, eb, kb2);
                    acc[c * NT + 0] = sk[0];
                    acc[c * NT + 1] = sk[1];
                    if (!EMRG) {
                        c6_skip(sk[0], 2, c, k_x, bias2, eb, kb2);
                        c6_unit(acc[c * NT + 2], acc[c * NT + 2], 1, c, k_y, eb, kb2);
                        acc[c * NT + 2] = sk[0];
                    } else if (c == CTW - 1) {                  // tile 2 of both channel tiles: every skip read before the unit writes
                        c6_skip(sk[0], 2, 0, k_x, bias2, eb, kb2);
                        c6_skip(sk[1], 2, 1, k_x, bias2, eb, kb2);
                        c6_unit(acc[0 * NT + 2], acc[1 * NT + 2], 2, 0, k_y, eb, kb2);
                        acc[0 * NT + 2] = sk[0];
                        acc[1 * NT + 2] = sk[1];
                    }
                } else if (YF) {
#pragma unroll
                    for (int pp = 0; pp < 2; ++pp) {
                        f32x16 sk[2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            if (h == 1 && pp == 1) break;
                            const int tt = pp == 0 ? h : 2;
                            const int q = tt * 32 + ln2;
                            const int key = q < 90 ? q : 89;
                            rb8::f32x32 xl;
                            if (xf) {                           // this lane's elements of the x_lo piece of the channel tile
                                const int c0 = 4 * (tc >> 1) + 2 * (tc & 1);
                                const u4 hd4 = *reinterpret_cast<const u4*>(lds + PSTR + choff(bd, key, c0));
                                const c8k::u32x2 tl2 = *reinterpret_cast<const c8k::u32x2*>(lds + PSTR + choff(bd, key, c0 + 1));
                                const uint32_t wv[7] = {hd4.x, hd4.y, hd4.z, hd4.w, tl2.x, tl2.y, 0u};
                                const uint32_t sh6 = (uint32_t)kb2 * 6u;
                                rb8::u32x6 pc;
#pragma unroll
                                for (int w = 0; w < 6; ++w) pc[w] = __builtin_amdgcn_alignbit(wv[w + 1], wv[w], sh6);
                                xl = __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(pc, __builtin_ldexpf(1.0f, k_x - cf8::X_LO_SHIFT));
                            }
#pragma unroll
                            for (int gg = 0; gg < 4; ++gg) {
                                const int chn = tc * 32 + gg * 8 + kb2 * 4;
                                const float4 bv = *reinterpret_cast<const float4*>(bias2 + chn);
                                float vv[4] = {bv.x, bv.y, bv.z, bv.w};
                                if (xf) {
                                    const Quad<_Float16> xq = *reinterpret_cast<const Quad<_Float16>*>(lds + choff(bd, key, chn >> 3) + (chn & 7) * 2);
#pragma unroll
                                    for (int i = 0; i < 4; ++i) vv[i] += (float)xq.e[i] + xl[2 * (gg * 4 + i)];
                                } else {                        // (the tower's first c6 block: the input layer's c8 image)
                                    int ox, oxl, oxh;
                                    offs(key, chn, ox, oxl, oxh);
                                    cf8::add_pair4(vv, *reinterpret_cast<const Quad<_Float16>*>(lds + ox), *reinterpret_cast<const uint32_t*>(lds + oxl));
                                }
#pragma unroll
                                for (int i = 0; i < 4; ++i) sk[h][gg * 4 + i] = vv[i];
                            }
                        }
                        if (pp == 0) {
                            write_c6_unit(acc[c * NT + 0], acc[c * NT + 1], tc, 0, k_y, ln2, kb2);
                            acc[c * NT + 0] = sk[0];
                            acc[c * NT + 1] = sk[1];
                        } else {
                            write_c6_unit(acc[c * NT + 2], acc[c * NT + 2], tc, 1, k_y, ln2, kb2);
                            acc[c * NT + 2] = sk[0];
                        }
                    }
                } else {
                    static_assert(YF || !XF, "a c8 intermediate image behind a c6 input does not exist");
#pragma unroll
                    for (int p = 0; p < NT; ++p) {
                        const int q = p * 32 + ln2;
                        const int key = q < 90 ? q : 89;
#pragma unroll
                        for (int gg = 0; gg < 4; ++gg) {
                            const int chn = tc * 32 + gg * 8 + kb2 * 4;
                            int ox, oxl, oxh;
                            offs(key, chn, ox, oxl, oxh);
                            const float4 bv = *reinterpret_cast<const float4*>(bias2 + chn);
                            float vv[4] = {bv.x, bv.y, bv.z, bv.w};
                            cf8::add_pair4(vv, *reinterpret_cast<const Quad<_Float16>*>(lds + ox), *reinterpret_cast<const uint32_t*>(lds + oxl));
                            float r[4];
#pragma unroll
                            for (int i = 0; i < 4; ++i) r[i] = ip4::relu1<(EP & 1) != 0>(acc[c * NT + p][gg * 4 + i]);
                            const cf8::Split4 o = cf8::split4(r);
                            if (q < 90) {
                                *reinterpret_cast<Quad<_Float16>*>(lds + ox) = o.hi;
                                *reinterpret_cast<uint32_t*>(lds + oxl) = o.l8;
                                *reinterpret_cast<uint32_t*>(lds + oxh) = o.h8;
                            }
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc[c * NT + p][gg * 4 + i] = vv[i];
                        }
                    }
                }
            }
            IP4_STAMP(5);
            __syncthreads();                                    // B: the images hold the intermediate activation; block g's biases are consumed
            if ((PF & 4) && NB > 1) {
                if (tid < C) {                                  // (write_bias(g + 2), its loads made before epilogue 1)
                    float* dst = reinterpret_cast<float*>(lds + BIAS_OFF) + (g & 1) * 2 * C;
                    dst[tid] = nb1;
                    dst[C + tid] = nb2;
                }
            } else if (NB > 1) write_bias(g + 2);
            IP4_STAMP(6);
            __builtin_amdgcn_s_setprio(3);
            if (!(PF & 1)) IP4_KLOOP(YF, flt2, 127 + k_y - cf8::X_LO_SHIFT, 127 + k_y, 7);
            else c8k::kloop_ctw_run<CTW, NT, C, YF, decltype(IP4_HOOK(7)), 3 ^ K2E>(lds, img, flt2, frags, lane, acc, 127 + k_y - cf8::X_LO_SHIFT, 127 + k_y, IP4_HOOK(7));
            if (CZ_IP4_VGPR_FORM) ip4::mfma_settle<CTW * NT>(acc);
            __builtin_amdgcn_s_setprio(0);
            IP4_STAMP(8);
            __syncthreads();                                    // K2: both waves of a board have read it
            IP4_STAMP(9);
            asm volatile("" : "+v"(ln2), "+v"(kb2));
            // in flight under epilogue 2 and the exit: the next block's K loop 1 fragments (behind the last block: block 0's,
            // for the next pair)
            if (PF & 16) issue_k1(blk_next);
            // epilogue 2: relu(acc) -> the operand triple over the image, or fp32 straight to HBM for the last block of a tower
            const int ex = blk == NB - 1 ? exit_mode : 0;
            if (EADR && ex != 0) {
                EpiBases es;
                epi_bases(es, ln2, kb2, false, true);
#pragma unroll
                for (int c = 0; c < CTW; ++c)
#pragma unroll
                    for (int p = 0; p < NT; ++p)
                        if (EDMP || p < 2 || es.ok2) {
#pragma unroll
                            for (int gg = 0; gg < 4; ++gg) {
                                float r[4];
#pragma unroll
                                for (int i = 0; i < 4; ++i) r[i] = ip4::relu1<(EP & 1) != 0>(acc[c * NT + p][gg * 4 + i]);
                                *reinterpret_cast<float4*>(lds + (es.s[p] ^ ((8 * c + 2 * gg) << 4))) = make_float4(r[0], r[1], r[2], r[3]);
                            }
                        }
            } else if (C == 128 && ex != 0) {
#pragma unroll
                for (int c = 0; c < CTW; ++c)
#pragma unroll
                    for (int p = 0; p < NT; ++p) {
                        const int q = p * 32 + ln2;
                        if (q < 90) {
#pragma unroll
                            for (int gg = 0; gg < 4; ++gg) {
                                const int chn = (tile0 + c) * 32 + gg * 8 + kb2 * 4;
                                float r[4];
#pragma unroll
                                for (int i = 0; i < 4; ++i) r[i] = ip4::relu1<(EP & 1) != 0>(acc[c * NT + p][gg * 4 + i]);
                                *reinterpret_cast<float4*>(lds + stg(q, chn)) = make_float4(r[0], r[1], r[2], r[3]);
                            }
                        }
                    }
            } else if (EC6U && !yf && k_out != CZ_C6_OUT_C8) {
                EpiBases eb2;
                epi_bases(eb2, ln2, kb2, true, false);
#pragma unroll
                for (int c = 0; c < CTW; ++c) {
                    c6_unit(acc[c * NT + 0], acc[c * NT + 1], 0, c, k_out, eb2, kb2);
                    if (!EMRG) c6_unit(acc[c * NT + 2], acc[c * NT + 2], 1, c, k_out, eb2, kb2);
                }
                if (EMRG) c6_unit(acc[0 * NT + 2], acc[1 * NT + 2], 2, 0, k_out, eb2, kb2);
            } else
#pragma unroll
            for (int c = 0; c < CTW; ++c) {
                const int tc = tile0 + c;
                if (YF && !yf && k_out != CZ_C6_OUT_C8) {
                    write_c6_unit(acc[c * NT + 0], acc[c * NT + 1], tc, 0, k_out, ln2, kb2);
                    write_c6_unit(acc[c * NT + 2], acc[c * NT + 2], tc, 1, k_out, ln2, kb2);
                } else {
#pragma unroll
                    for (int p = 0; p < NT; ++p) {
                        const int q = p * 32 + ln2;
                        const int board = 2 * t + bd;
                        if (q < 90) {
#pragma unroll
                            for (int gg = 0; gg < 4; ++gg) {
                                const int chn = tc * 32 + gg * 8 + kb2 * 4;
                                float r[4];
#pragma unroll
                                for (int i = 0; i < 4; ++i) r[i] = ip4::relu1<(EP & 1) != 0>(acc[c * NT + p][gg * 4 + i]);
                                if (yf) {
                                    if (board < n_boards)
                                        *reinterpret_cast<float4*>(yf + ((size_t)board * 90 + q) * C + chn) = make_float4(r[0], r[1], r[2], r[3]);
                                } else {
                                    int ox, oxl, oxh;
                                    offs(q, chn, ox, oxl, oxh);
                                    const cf8::Split4 o = cf8::split4(r);
                                    *reinterpret_cast<Quad<_Float16>*>(lds + ox) = o.hi;
                                    *reinterpret_cast<uint32_t*>(lds + oxl) = o.l8;
                                    *reinterpret_cast<uint32_t*>(lds + oxh) = o.h8;
                                }
                            }
                        }
                    }
                }
            }
            IP4_STAMP(10);
            __syncthreads();                                    // C: the result is in the images
            IP4_STAMP(11);
        }
#ifdef CZ_IP4_STAMPS
        const int blk = NB - 1;                                 // (the pair's own phases: in the last block's row)
#endif
        // in flight under the exit (PF & 32): the workgroup's next pair.  The exit stands behind the block loop, so that the
        // request's registers are live from here to the store behind the barrier below and nowhere in the loop.
        u4 nxt[2][LITER];
        if (FE && t + stride < n_pairs) fill_request(t + stride, nxt);
        {
            const int ex = exit_mode;
            if (C == 128 && ex != 0) {
                // the exit of board 2 t + bd by its two waves: item i = (pixel i >> 2, 32-channel block i & 3)
                const int board = 2 * t + bd;
                struct alignas(16) H8 { Quad<_Float16> a, b; };
                const float* hwl = reinterpret_cast<const float*>(lds + HW_OFF);
#pragma unroll
                for (int it = 0; it < 3; ++it) {
                    const int i = it * 128 + (wave & 1) * 64 + lane;
                    if (i >= 90 * 4) continue;
                    const int qq = i >> 2, b32 = i & 3;
                    if (ex == IP4_EXIT_PAIRS) {
                        if (board >= n_boards) continue;
                        const size_t ebase = (size_t)board * 90 * C;
                        _Float16* yl = reinterpret_cast<_Float16*>(yc);
                        // (PF & 8: a step's two quads are read while the step before is converted and stored)
                        float4 fq[2][2];
                        auto ld = [&](int k8) {
                            fq[k8 & 1][0] = *reinterpret_cast<const float4*>(lds + stg(qq, b32 * 32 + 8 * k8));
                            fq[k8 & 1][1] = *reinterpret_cast<const float4*>(lds + stg(qq, b32 * 32 + 8 * k8 + 4));
                        };
                        if (PF & 8) ld(0);
#pragma unroll
                        for (int k8 = 0; k8 < 4; ++k8) {
                            if (!(PF & 8)) ld(k8);
                            else if (k8 + 1 < 4) {
                                ld(k8 + 1);
                                __builtin_amdgcn_sched_barrier(0);
                            }
                            const float4 f0 = fq[k8 & 1][0], f1 = fq[k8 & 1][1];
                            const float r[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                            H8 hi, lo;
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                hi.a.e[j] = (_Float16)r[j];
                                hi.b.e[j] = (_Float16)r[4 + j];
                                lo.a.e[j] = (_Float16)(r[j] - (float)hi.a.e[j]);
                                lo.b.e[j] = (_Float16)(r[4 + j] - (float)hi.b.e[j]);
                            }
                            reinterpret_cast<u4*>(yh + ebase)[qq * 16 + b32 * 4 + k8] = __builtin_bit_cast(u4, hi);
                            reinterpret_cast<u4*>(yl + ebase)[qq * 16 + b32 * 4 + k8] = __builtin_bit_cast(u4, lo);
                            if (PF & 8) __builtin_amdgcn_sched_barrier(0);
                        }
                    } else {
                        float a6[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
                        if (PF & 8) {
                            // a step's feature quad and six weight quads in registers of their own, the next step's requested
                            // before this one's arithmetic; the six sums side by side, each in the plain loop's order
                            float4 fq[2], wq[2][6];
                            auto ld = [&](int k4) {
                                fq[k4 & 1] = *reinterpret_cast<const float4*>(lds + stg(qq, b32 * 32 + 4 * k4));
#pragma unroll
                                for (int o = 0; o < 6; ++o)
                                    wq[k4 & 1][o] = *reinterpret_cast<const float4*>(hwl + o * C + b32 * 32 + 4 * k4);
                            };
                            ld(0);
#pragma unroll
                            for (int k4 = 0; k4 < 8; ++k4) {
                                if (k4 + 1 < 8) ld(k4 + 1);
                                __builtin_amdgcn_sched_barrier(0);
                                const float4 f = fq[k4 & 1];
#pragma unroll
                                for (int o = 0; o < 6; ++o) a6[o] += f.x * wq[k4 & 1][o].x;
#pragma unroll
                                for (int o = 0; o < 6; ++o) a6[o] += f.y * wq[k4 & 1][o].y;
#pragma unroll
                                for (int o = 0; o < 6; ++o) a6[o] += f.z * wq[k4 & 1][o].z;
#pragma unroll
                                for (int o = 0; o < 6; ++o) a6[o] += f.w * wq[k4 & 1][o].w;
                                __builtin_amdgcn_sched_barrier(0);
                            }
                        } else
#pragma unroll
                        for (int k4 = 0; k4 < 8; ++k4) {
                            const float4 f = *reinterpret_cast<const float4*>(lds + stg(qq, b32 * 32 + 4 * k4));
#pragma unroll
                            for (int o = 0; o < 6; ++o) {
                                const float4 w = *reinterpret_cast<const float4*>(hwl + o * C + b32 * 32 + 4 * k4);
                                a6[o] += f.x * w.x; a6[o] += f.y * w.y; a6[o] += f.z * w.z; a6[o] += f.w * w.w;
                            }
                        }
#pragma unroll
                        for (int o = 0; o < 6; ++o) {              // the four lanes of the pixel: (a0 + a1) + (a2 + a3) on every lane
                            a6[o] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(a6[o]), 0xB1, 0xF, 0xF, true));
                            a6[o] += __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(a6[o]), 0x4E, 0xF, 0xF, true));
                        }
                        if (board >= n_boards) continue;
#pragma unroll
                        for (int o = 0; o < 6; ++o)
                            if ((o & 3) == b32) {                   // lane b32 writes outputs b32 and b32 + 4
                                float hv = a6[o] + hd.b[o];
                                hv = hv > 0.0f ? hv : 0.0f;
                                if (o < hd.n_pol) hd.pol[(size_t)board * (hd.n_pol * 90) + o * 90 + qq] = hv;
                                else hd.val[(size_t)board * ((6 - hd.n_pol) * 90) + (o - hd.n_pol) * 90 + qq] = hv;
                            }
                    }
                }
            }
            IP4_STAMP(12);
        }
        if (!yf_last && exit_mode == 0) drain(t);
        IP4_STAMP(13);
        t += stride;
        if (t >= n_pairs) break;
        __syncthreads();                                        // (drain and the exit have read the images)
        if (FE) fill_store(nxt);
        else fill(t);
        IP4_STAMP(14);
    }
}

// the staged chains (c8 / c6 images): operands, the block list, one of the two outputs
struct ChainCall {
    const void *xh, *xc;
    const BlockChain<ip::MAX_BLOCKS>& ch;
    void *yh, *yc;
    float* yf;
    int n, n_cu;
    const int32_t* n_dev;
    hipStream_t st;
};

// a pair of boards per workgroup on four matrix waves of C / 64 channel tiles
template <int C, int XF, int YF, bool MIX = false>
void launch_ip4(const ChainCall& a, int exit_mode = 0, HeadArgs hd = HeadArgs{})
{
    hipLaunchKernelGGL((k_resblock_ip4_c8<C, XF, YF, MIX>), dim3(nn_grid((a.n + 1) / 2, a.n_cu)), dim3(256), 0, a.st,
                       (const _Float16*)a.xh, (const unsigned char*)a.xc, a.ch, (_Float16*)a.yh, (unsigned char*)a.yc, a.yf, a.n,
                       a.n_dev, exit_mode, hd);
}

}  // namespace
