// xq_conv_pack.hip -- the host side of the convolutions' filters: cz_conv3x3_pack_weights, cz_conv3x3_c8_pack_weights,
// cz_conv3x3_c6_pack_weights and cz_input_conv_pack_weights put a filter [O][I][kh][kw] into the order the kernels of csrc/xq_conv.hip,
// csrc/xq_conv_ip4.hip and csrc/xq_tower.hip stream it in (fragment order, the c8 / c6 correction pieces and their shifts behind it);
// cz_*_packed_elems / _bytes size the buffers.  Host code only: no kernel and no launch lives here.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <cmath>
#include "../../include/czero.h"
#include "xq_nn_common.h"       // W_PAD_STEPS, CZ_C6_OUT_C8
#include "xq_nn_launch.h"       // czi_set_error, the host bf16 / f16 conversions

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

// ---- c8 / c6 arithmetic (k_conv3x3_c8, k_resblock_c8 and the chains): packing ---------------------------------------------------
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
// A c8 / c6 packed filter of C channels: main_u4 uint4 of fp16 fragments, c8_u4 uint4 of correction pieces (c8k::Geo<C>::MAIN_U4,
// C8_U4: the kernels' side, held equal at compile time in k_conv3x3_c8), then 4 ints and 2 x C per-output-channel shifts (signed bytes)
struct C8Layout {
    size_t main_u4, c8_u4, bytes;
};
inline C8Layout c8_layout(int channels)
{
    const size_t C = (size_t)channels, KK = C / 16, CT = C / 32, NB = C / 64;
    C8Layout l;
    l.main_u4 = (9 * KK + W_PAD_STEPS) * CT * 64;
    l.c8_u4 = (9 * NB + 1) * 2 * CT * 2 * 64;
    l.bytes = (l.main_u4 + l.c8_u4 + 1) * 16 + 2 * C;
    return l;
}
}  // namespace

extern "C" size_t cz_conv3x3_c8_packed_bytes(int channels)
{
    if (channels != 128 && channels != 192) return 0;
    return c8_layout(channels).bytes;
}

extern "C" int cz_conv3x3_c8_pack_weights(const float* w_oihw, int channels, void* out_host)
{
    if (!w_oihw || !out_host || (channels != 128 && channels != 192)) {
        czi_set_error("cz_conv3x3_c8_pack_weights: bad argument (128 or 192 filters)");
        return CZ_ERR_ARG;
    }
    const int C = channels, KK = C / 16, CT = C / 32, NB = C / 64;
    const C8Layout lay = c8_layout(C);
    const size_t main_u4 = lay.main_u4, c8_u4 = lay.c8_u4;
    memset(out_host, 0, lay.bytes);
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
    const C8Layout lay = c8_layout(C);
    const size_t main_u4 = lay.main_u4, c8_u4 = lay.c8_u4;
    memset(out_host, 0, lay.bytes);
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
