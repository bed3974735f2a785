// xq_conv_kloop.h -- part of xq_conv.hip's translation unit; do not compile it into a second one: the unit's device code is
// compared kernel by kernel when text moves between these headers (EXPERIMENTS.md, "the convolution unit's text in headers"), and
// the search unit's kernels changed by 0.4-1.7 % when part of that unit was compiled alone.
//
// The shared K loop and the LDS image it reads: tile_load, tile_write, zero_rows_write, conv_kloop.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xq_nn_common.h"
#include "xq_conv_geom.h"

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

}  // namespace
