// xq_conv_geom.h -- the LDS image geometry and the in-place chains' row layout, shared by the translation units that hold the
// convolution kernels (csrc/xq_conv.hip, csrc/xq_conv_ip4.hip).  Anonymous namespace, as xq_nn_common.h: a copy per unit.
#pragma once
#include "xq_nn_common.h"

namespace {

// ---- geometry shared by both kernels -----------------------------------------------------------------------------
template <int C, int P, int PARTS> struct Geom {
    static constexpr int RB = C * 2;                 // bytes per pixel row in LDS
    static constexpr int CPR = RB / 16;              // 16-byte chunks per row
    static constexpr bool POW2 = (RB & (RB - 1)) == 0;        // 192 filters: 384-byte rows, 24 chunks
    // swizzle: chunk ^= row & SWZ.  It must stay inside the row: all chunks for power-of-two rows, an aligned group of 8
    // otherwise (two of the 16 rows of a read group then share a slot: a 2-way conflict instead of none)
    static constexpr int SWZ = POW2 ? (CPR - 1 < 15 ? CPR - 1 : 15) : 7;
    static_assert(POW2 || CPR % 8 == 0, "rows must be a whole number of 8-chunk groups");
    // byte offset of K-step kk relative to pre[] (= row * RB + ((kb ^ (row & SWZ)) << 4)): the chunk is 2 * kk + kb and
    // the XOR only touches the bits SWZ covers, the rest of 2 * kk is a plain add
    static __device__ __forceinline__ int kstep(int pre, int kk)
    {
        if (POW2) return pre ^ (kk << 5);
        return (pre ^ ((kk & 3) << 5)) + ((kk >> 2) << 7);
    }
    // 16 all-zero rows for out-of-board taps and padding pixels.  A lane whose tap leaves the board reads zero row
    // ZROW + (r & 15), r = the row it would have read: every ds_read_b128 lane group (16 lanes, MI355X_MICROARCH.md
    // section LDS) covers 16 consecutive values of r, so its 16 lanes -- on the board or not -- keep 16 distinct
    // (row & 15), i.e. 16 distinct 16-byte slots of the 256-byte bank row.  (One shared zero row cost a 2-way conflict in
    // almost every group that had an off-board lane: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.36 in round 1.)
    static constexpr int ZROW = (P * 90 + 15) / 16 * 16;
    static constexpr int ZROWS = 16;
    static constexpr int PART_BYTES = (ZROW + ZROWS) * RB;
    static constexpr int REGION = PARTS * PART_BYTES;
    static constexpr int NT = P * 3;                 // pixel tiles of 32 (96 slots per board, 90 used)
    static constexpr int KK = C / 16;                // K-steps per tap
    static constexpr int CT = C / 32;                // channel tiles = waves per board group
    static constexpr int GTHREADS = CT * 64;
    static constexpr int CHUNKS = P * 90 * CPR;      // 16-byte chunks per part
    static constexpr int ITER = (CHUNKS + GTHREADS - 1) / GTHREADS;
    static constexpr int W_STEP = CT * 64;           // uint4 per K-step of packed weights
    static constexpr int W_RING = KK < W_RING_MAX ? KK : W_RING_MAX;   // ring slot = step % W_RING
    static constexpr int W_PART = (9 * KK + W_PAD_STEPS) * W_STEP;
    static_assert(KK % W_RING == 0 && KK % 2 == 0, "ring / double-buffer indices are taken from kk");
};

// the in-place residual-block kernels (k_resblock_ip, k_resblock_ip_c8, k_resblock_ip4_c8): rows of the X and Y images, the
// zero rows behind them
namespace ip {
constexpr int ROW_Y = 90, ROW_Z = 192, ROWS = ROW_Z + 16, COPY_THREADS = 128;       // (ROW_Z: a multiple of 16)
constexpr int MAX_BLOCKS = 12;       // k_resblock_ip_c8: the consecutive blocks a launch takes every board through (1 .. 12)
}

}  // namespace
