// xq_nn_launch.h -- the host side the network entry points share (csrc/xq_conv.hip, csrc/xq_conv_ip4.hip, csrc/xq_tower.hip, csrc/xq_heads.hip): error
// returns, the CU count, grid sizes, the end of a launch, the chain argument's fill, the compact queue's context, the host
// bf16 / f16 conversions of the packers and the prototypes of the two launches that cross translation units.  Host code only;
// like xq_nn_common.h everything but those prototypes sits in an anonymous namespace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/czero.h"
#include "xq_nn_common.h"

extern "C" void czi_set_error(const char* msg);

// The launches on the four-wave pair kernels, which live in one translation unit and are reached from both.  `name`: the entry
// point, for nn_launched().  n_cu: nn_cu_count()'s.
// csrc/xq_conv_ip4.hip, k_resblock_ip4_c8<128>: a chain of 128-filter blocks of one staged arithmetic (c6: 1, c8: 0); exit_mode: 0 =
// the operand pair (c6 image, or the c8 image a c6 chain hands over), IP4_EXIT_PAIRS, IP4_EXIT_HEADS.
extern "C" int czi_tower4_launch(const char* name, const void* x_hi, const void* x_img, const BlockChain<12>* ch, int c6,
                                 int exit_mode, void* y_hi, void* y_img, const float* head_w, const float* head_b, float* pol,
                                 float* val, int n_pol, int n_boards, int n_cu, const int32_t* n_dev, void* stream);
// csrc/xq_tower.hip, k_tower_pairs4<E, channels>: (hi, lo) pair blocks at 128 filters (heads exit: head_w != NULL) or 192 (y_f32
// != NULL: the last block writes fp32).
extern "C" int czi_pairs4_launch(const char* name, const void* x_hi, const void* x_lo, const BlockChain<12>* ch, void* y_hi,
                                 void* y_lo, const float* head_w, const float* head_b, float* pol, float* val, int n_pol,
                                 int n_boards, int channels, int dtype, int n_cu, const int32_t* n_dev, void* stream,
                                 float* y_f32);

namespace {

// The compact evaluation queue, which is all that tells a _q entry point from its plain form: the kernels take the board count
// as min(n_boards, *n_dev) on the device, and the input layer reads board i from planes[rows[i]].  NULL: n_boards / identity.
struct QueueCtx {
    const int32_t* rows;
    const int32_t* n_dev;
};

inline int nn_error(int rc, const char* msg)
{
    czi_set_error(msg);
    return rc;
}

inline int nn_error(int rc, const char* name, const char* what)       // "<name>: <what>"
{
    char msg[256];
    snprintf(msg, sizeof(msg), "%s: %s", name, what);
    return nn_error(rc, msg);
}

// compute units of the current device (asked once); < 0 with "<name>: cannot query the device" set when it cannot be had
inline int nn_cu_count(const char* name)
{
    static int n_cu = 0;
    if (n_cu == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess)
            return nn_error(CZ_ERR_HIP, name, "cannot query the device");
        n_cu = prop.multiProcessorCount;
    }
    return n_cu;
}

// persistent kernels: one workgroup per unit of work (board, pair, tile), at most one per CU
inline unsigned nn_grid(int units, int n_cu) { return (unsigned)(units < n_cu ? units : n_cu); }

// the end of an entry point that has launched: CZ_OK, or CZ_ERR_HIP with "<name>: launch failed"
inline int nn_launched(const char* name)
{
    return hipGetLastError() == hipSuccess ? CZ_OK : nn_error(CZ_ERR_HIP, name, "launch failed");
}

// CZ_IP_PAIR=0: the 192-filter staged blocks run one board on six matrix waves (k_resblock_ip_c8) instead of a pair of boards
// on four waves of three channel tiles (k_resblock_ip4_c8).  A/B runs; read at every call, the tests run both in one process.
inline bool nn_ip_pair()
{
    const char* e = getenv("CZ_IP_PAIR");
    return !(e && e[0] == '0');
}

// Blocks [first, n) of the per-block arrays into ch (n: 1 .. MAX, checked by the caller); a NULL among them: false, with
// "<name>: null block parameter" set.
template <int MAX>
inline bool fill_chain(BlockChain<MAX>& ch, const char* name, int n, const void* const* w1, const float* const* b1,
                       const void* const* w2, const float* const* b2, int first = 0)
{
    ch.n = n;
    for (int b = first; b < n; ++b) {
        if (!w1[b] || !w2[b] || !b1[b] || !b2[b]) {
            nn_error(CZ_ERR_ARG, name, "null block parameter");
            return false;
        }
        ch.w1[b] = w1[b]; ch.w2[b] = w2[b]; ch.b1[b] = b1[b]; ch.b2[b] = b2[b];
    }
    return true;
}

// round-to-nearest-even conversions on the host (the weight packers)
inline uint16_t f32_to_bf16_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_bits_to_f32(uint16_t h)
{
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline uint16_t f32_to_f16_bits(float f)
{
    const _Float16 h = (_Float16)f;
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}
inline float f16_bits_to_f32(uint16_t b)
{
    _Float16 h;
    memcpy(&h, &b, 2);
    return (float)h;
}

}  // namespace
