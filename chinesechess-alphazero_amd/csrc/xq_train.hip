// xq_train.hip -- the trainer's data path and loss for gfx950 (run.py opt, worker/optimize.py) + their C-ABI entry points.
//
//   k_replay_games       one wavefront per game replays all of a record's plies (the boards of expanding_data,
//                        reference worker/optimize.py:234-258) with step_board, the move application of k_step
//   k_gather_planes      one wavefront per minibatch row: window index -> 14 or 28 float32 input planes (state_to_planes /
//                        state_history_to_planes, environment/static_env.py:137-194) with wave_encode, the encoder of k_encode
//   k_policy_value_loss  one wavefront per minibatch row: softmax, Keras 2.0.8's clipped categorical cross-entropy against the
//                        played move's one-hot or the record's visit counts, squared value error, and their gradients;
//                        <WDL = true> (cz_policy_wdl_loss): the same policy half, and for a win / draw / loss value head the
//                        clipped cross-entropy of its three logits against the class of z, with its gradient
//                        <MASK = true> (cz_policy_value_loss_l / cz_policy_wdl_loss_l, run.py opt --policy-mask legal): the
//                        softmax, the loss and the gradient run over the row's legal moves (and its target's support) only;
//                        the row's wavefront generates the mask from the window's board with wave_movegen
//   k_moves_left_loss    one thread per minibatch row (cz_moves_left_loss, run.py opt --moves-left): Huber loss of softplus(x)
//                        against the row's plies-to-the-end target in units of 32 plies, and its gradient
//
// Mirror augmentation (run.py opt --augment mirror): both per-step kernels take an optional per-row flag array.  A flagged
// row is the left-right mirror image of its position (file x <-> 8 - x, a symmetry of the rules): its board is mirrored in
// LDS before the one encoder runs, and its target labels go through the label mirror M before they are scattered into the
// row's dense target.  The flag is the same for the 64 lanes of a row's wavefront, so the branch is wave-uniform; a NULL
// array is the unflagged kernel.
//
// The legal-move mask (run.py opt --policy-mask legal): the search normalises a node's priors over its legal moves alone
// (xq_search_attach.h: logits_to_weights), so the masked loss trains that distribution.  The window keeps every position's
// board in the mover's frame, the frame of the labels: the row's wavefront loads it (mirrored when the row is flagged), runs
// wave_movegen and marks the list's labels in a byte mask in LDS.  A column outside the mask and outside the target's support
// is read as -inf; everything after that is the unmasked code, so the masked kernel on x gives the bits of the unmasked one
// on x with those columns set to -inf.  No dense mask tensor exists and no host rule code runs in a step.
//
// The contract (shapes, order, error reporting, bit-identity) is stated in include/czero.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "xq_rules.h"
#include "xq_mirror.h"
#include "../../include/czero.h"

using namespace xq;

extern "C" void czi_set_error(const char* msg);

namespace {

inline int grid_for(int n)
{
    const int cap = 256 * 32;            // as xq_kernels.hip: 256 CUs x up to 32 single-wave workgroups, the rest grid-stride
    return n < cap ? (n > 0 ? n : 1) : cap;
}

int launch_status(const char* what)
{
    if (hipGetLastError() != hipSuccess) {
        czi_set_error(what);
        return CZ_ERR_HIP;
    }
    return CZ_OK;
}

XQ_D float wave_sum_f32(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);   // every lane ends with the same bits
    return v;
}

XQ_D double wave_sum_f64(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

XQ_D int wave_sum_i32(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

XQ_D void zero_planes(float* __restrict__ out)   // 14 planes: 315 float4
{
    for (int q = lane_id(); q < 315; q += 64) reinterpret_cast<float4*>(out)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

constexpr int LOSS_COLS = (NLABELS + 63) / 64;       // 33 logits per lane
constexpr float CCE_EPS = 1e-7f;                     // Keras 2.0.8 epsilon(); the upper clip is float(1 - 1e-7)
constexpr float CCE_HI = (float)(1.0 - 1e-7);

// Per-wave LDS of the legal-move mask (k_policy_value_loss<WDL, true>): the row's board, its move list and the mask itself,
// one byte per label column (a byte store needs no atomic where two moves carry one label).
struct alignas(16) MaskLDS {
    int8_t bd[BOARD_LDS];
    MoveList ml;
    uint16_t plist[BOARD_LDS];
    uint8_t legal[LOSS_COLS * 64];
};

// legal[j] = 1 for every label of the move list of board `g` (mirrored first when mir), 0 elsewhere.  The list holds up to
// MAXMOVES = 128 entries: a lane marks entry lane and entry lane + 64.
XQ_D void mark_legal(const int8_t* __restrict__ g, bool mir, MaskLDS& m)
{
    const int lane = lane_id();
    load_board(g, m.bd);
    if (mir) mirror_board(m.bd);
    int n = wave_movegen(m.bd, m.ml, m.plist);
    n = n < MAXMOVES ? n : MAXMOVES;
    for (int q = lane; q < LOSS_COLS * 16; q += 64) reinterpret_cast<uint32_t*>(m.legal)[q] = 0u;
    wave_sync();
    for (int k = lane; k < n; k += 64) {
        const int lab = m.ml.lab[k];
        if (lab < NLABELS) m.legal[lab] = 1;
    }
    wave_sync();
}

}  // namespace

__global__ __launch_bounds__(64) void k_replay_games(const int8_t* __restrict__ init, const uint16_t* __restrict__ labels,
                                                    const int32_t* __restrict__ offsets, int n_games, int n_pos,
                                                    int8_t* __restrict__ boards, int32_t* __restrict__ prev,
                                                    int32_t* __restrict__ bad)
{
    __shared__ int8_t bd[2][BOARD_LDS];
    const int lane = lane_id();
    for (int g = blockIdx.x; g < n_games; g += gridDim.x) {
        const int o0 = offsets[g], o1 = offsets[g + 1];
        if (o0 < 0 || o1 < o0 || o1 > n_pos) {           // nothing written for a game whose span is not inside [0, n_pos)
            if (lane == 0) bad[g] = -2;
            continue;
        }
        load_board(init + (size_t)g * NSQ, bd[0]);
        int cur = 0, bad_ply = -1;
        for (int t = o0; t < o1; ++t) {
            store_board(bd[cur], boards + (size_t)t * NSQ);
            if (lane == 0) prev[t] = t - o0 >= 2 ? t - 2 : -1;
            if (bad_ply >= 0) continue;                  // after an invalid move the board stays as it was (as cz_step)
            const int label = labels[t];
            bool moved = false;
            if (label < NLABELS) {
                const int ft = label_ft(label);
                const int f = ft >> 8, to = ft & 0xFF;
                if (bd[cur][f] != 0) {
                    step_board(bd[cur], f, to, bd[cur ^ 1]);
                    cur ^= 1;
                    moved = true;
                }
            }
            if (!moved) bad_ply = t - o0;
        }
        if (lane == 0) bad[g] = bad_ply;
        wave_sync();
    }
}

__global__ __launch_bounds__(64) void k_gather_planes(const int8_t* __restrict__ boards, const int32_t* __restrict__ prev,
                                                     int n_pos, const int32_t* __restrict__ idx,
                                                     const uint8_t* __restrict__ mirror, int n_rows, int depth,
                                                     float* __restrict__ planes)
{
    __shared__ int8_t bd[BOARD_LDS];
    for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int i = idx[r];
        const bool mir = mirror != nullptr && mirror[r] != 0;   // wave-uniform: one row, one wavefront
        float* out = planes + (size_t)r * depth * 90;
        if (i < 0 || i >= n_pos) {                       // out-of-range index: zero planes, nothing read
            zero_planes(out);
            if (depth == 28) zero_planes(out + 1260);
            continue;
        }
        load_board(boards + (size_t)i * NSQ, bd);
        if (mir) mirror_board(bd);
        wave_encode<0>(bd, out);
        if (depth == 28) {
            const int p = prev[i];
            if (p >= 0 && p < n_pos) {
                wave_sync();
                load_board(boards + (size_t)p * NSQ, bd);
                if (mir) mirror_board(bd);
                wave_encode<0>(bd, out + 1260);
            } else {
                zero_planes(out + 1260);
            }
        }
        wave_sync();
    }
}

template <bool WDL, bool MASK>
__global__ __launch_bounds__(64) void k_policy_value_loss(
    const float* __restrict__ logits, int ld, const float* __restrict__ v, const int32_t* __restrict__ idx,
    const uint8_t* __restrict__ mirror, int n_rows, int n_pos, const int32_t* __restrict__ row_ptr, const uint16_t* __restrict__ vis_label,
    const int32_t* __restrict__ vis_count, int nnz, const uint16_t* __restrict__ played, const float* __restrict__ z,
    const float* __restrict__ q, float q_ratio, const float* __restrict__ row_w, int mode,
    float w_p, float w_v, float* __restrict__ policy_loss, float* __restrict__ value_sqerr,
    float* __restrict__ grad_logits, float* __restrict__ grad_v, float* __restrict__ value_ce,
    const int8_t* __restrict__ boards, int32_t* __restrict__ off_mask, float* __restrict__ illegal_mass,
    float* __restrict__ illegal_margin)                // the last four: MASK only
{
    __shared__ float tgt[LOSS_COLS * 64];            // the row's dense target, built from the sparse entries
    __shared__ MaskLDS mk;                           // MASK only: never named otherwise, and then not allocated
    const int lane = lane_id();
    const float inv_b = 1.0f / (float)n_rows;
    const float c = w_p * inv_b;
    for (int r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const int i = idx[r];
        const bool mir = mirror != nullptr && mirror[r] != 0;   // wave-uniform: one row, one wavefront
        float* g = grad_logits + (size_t)r * NLABELS;
        if (i < 0 || i >= n_pos) {                       // out-of-range index: zero loss and gradient, nothing read
            for (int j = lane; j < NLABELS; j += 64) g[j] = 0.f;
            if (lane == 0) {
                policy_loss[r] = 0.f;
                value_sqerr[r] = 0.f;
                if (WDL) {
                    value_ce[r] = 0.f;
                    grad_v[3 * r] = grad_v[3 * r + 1] = grad_v[3 * r + 2] = 0.f;
                } else {
                    grad_v[r] = 0.f;
                }
                if constexpr (MASK) {
                    if (off_mask != nullptr) off_mask[r] = 0;
                    if (illegal_mass != nullptr) illegal_mass[r] = 0.f;
                    if (illegal_margin != nullptr) illegal_margin[r] = 0.f;
                }
            }
            continue;
        }
        if constexpr (MASK) mark_legal(boards + (size_t)i * NSQ, mir, mk);
#pragma unroll
        for (int k = 0; k < LOSS_COLS; ++k) tgt[lane + 64 * k] = 0.f;
        wave_sync();
        // row weight (cz_policy_value_loss_w): scales the row's gradients only; 1.0f leaves every bit where it was
        const float wi = row_w != nullptr ? row_w[i] : 1.f;
        const float cr = row_w != nullptr ? __fmul_rn(c, wi) : c;
        double total = 0.0;
        int lo = 0, hi = 0;
        if (mode == 1 && nnz > 0) {
            lo = row_ptr[i];
            hi = row_ptr[i + 1];
            if (lo < 0 || hi > nnz || hi < lo) lo = hi = 0;   // a span outside [0, nnz): no visits, nothing read
            for (int k = lo + lane; k < hi; k += 64) total += (double)vis_count[k];
            total = wave_sum_f64(total);
        }
        if (total > 0.0) {
            for (int k = lo + lane; k < hi; k += 64) {
                int lab = vis_label[k];
                if (mir && lab < NLABELS) lab = mirror_label(lab);
                if (lab < NLABELS) tgt[lab] = (float)((double)vis_count[k] / total);   // float64 quotient, rounded once
            }
        } else if (lane == 0) {
            int lab = played[i];
            if (mir && lab < NLABELS) lab = mirror_label(lab);
            if (lab < NLABELS) tgt[lab] = 1.f;
        }
        wave_sync();
        // softmax over the row, max subtracted, all in fp32
        const float* zr = logits + (size_t)r * ld;
        float e[LOSS_COLS];
        float mx = -INFINITY;
        uint64_t in_a = 0;                               // MASK: bit k = this lane's column lane + 64 k is in A
        int off = 0;                                     // MASK: this lane's target entries outside the legal set
#pragma unroll
        for (int k = 0; k < LOSS_COLS; ++k) {
            const int j = lane + 64 * k;
            e[k] = j < NLABELS ? zr[j] : -INFINITY;
            if constexpr (MASK) {
                // A = the legal labels and the target's support; a column outside A is read as -inf, whatever it holds
                const bool legal = mk.legal[j] != 0, sup = tgt[j] != 0.f;
                if (legal || sup) in_a |= 1ull << k;
                else e[k] = -INFINITY;
                off += (sup && !legal) ? 1 : 0;
            }
            mx = fmaxf(mx, e[k]);
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 64));
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < LOSS_COLS; ++k) {
            const int j = lane + 64 * k;
            e[k] = j < NLABELS ? expf(e[k] - mx) : 0.f;
            s += e[k];
        }
        s = wave_sum_f32(s);
        // loss = -sum t log(clip(p)); S = sum t m, m = 1 where the clip passes the gradient (eps < p < 1 - eps)
        float loss = 0.f, S = 0.f;
#pragma unroll
        for (int k = 0; k < LOSS_COLS; ++k) {
            const float p = e[k] / s;
            e[k] = p;
            const float t = tgt[lane + 64 * k];
            if (t != 0.f) {
                const float pc = fminf(fmaxf(p, CCE_EPS), CCE_HI);
                loss -= t * logf(pc);
                if (p > CCE_EPS && p < CCE_HI) S += t;
            }
        }
        loss = wave_sum_f32(loss);
        S = wave_sum_f32(S);
#pragma unroll
        for (int k = 0; k < LOSS_COLS; ++k) {
            const int j = lane + 64 * k;
            if (j < NLABELS) {
                const float p = e[k];
                const float tm = (p > CCE_EPS && p < CCE_HI) ? tgt[j] : 0.f;
                g[j] = cr * (p * S - tm);
            }
        }
        if constexpr (MASK) {
            off = wave_sum_i32(off);
            if (off_mask != nullptr && lane == 0) off_mask[r] = off;
            if (illegal_mass != nullptr || illegal_margin != nullptr) {
                // validation only (a training step passes NULL): the logits are read again, L2 still holds them.
                // mo = the largest logit outside A; the full softmax over all 2086 columns has its maximum max(mx, mo).
                float mo = -INFINITY;
#pragma unroll
                for (int k = 0; k < LOSS_COLS; ++k) {
                    const int j = lane + 64 * k;
                    if (j < NLABELS && !((in_a >> k) & 1ull)) mo = fmaxf(mo, zr[j]);
                }
#pragma unroll
                for (int m = 32; m >= 1; m >>= 1) mo = fmaxf(mo, __shfl_xor(mo, m, 64));
                const float mf = fmaxf(mx, mo);
                double s_in = 0.0, s_out = 0.0;          // fp32 exponentials, summed in float64
#pragma unroll
                for (int k = 0; k < LOSS_COLS; ++k) {
                    const int j = lane + 64 * k;
                    if (j < NLABELS) {
                        const double ex = (double)expf(zr[j] - mf);
                        if ((in_a >> k) & 1ull) s_in += ex;
                        else s_out += ex;
                    }
                }
                s_in = wave_sum_f64(s_in);
                s_out = wave_sum_f64(s_out);
                if (lane == 0) {
                    if (illegal_mass != nullptr) illegal_mass[r] = (float)(s_out / (s_in + s_out));
                    if (illegal_margin != nullptr) illegal_margin[r] = mo - mx;
                }
            }
        }
        if (WDL) {
            // v: the row's three value logits (win, draw, loss); the target class is the sign of z.  The same softmax, clip
            // and gradient mask as the policy half above, on a one-hot target: grad_k = p_k S - t_k m_k with S = m_target.
            if (lane == 0) {
                const float zi = z[i];
                const int tc = zi > 0.f ? 0 : (zi < 0.f ? 2 : 1);
                const float l0 = v[3 * r], l1 = v[3 * r + 1], l2 = v[3 * r + 2];
                const float vm = fmaxf(fmaxf(l0, l2), l1);
                const float e0 = expf(l0 - vm), e1 = expf(l1 - vm), e2 = expf(l2 - vm);
                const float vs = (e0 + e2) + e1;
                const float p[3] = {e0 / vs, e1 / vs, e2 / vs};
                const float pt = tc == 0 ? p[0] : (tc == 1 ? p[1] : p[2]);
                const float Sv = (pt > CCE_EPS && pt < CCE_HI) ? 1.f : 0.f;
                const float d = (p[0] - p[2]) - zi;
                policy_loss[r] = loss;
                value_sqerr[r] = d * d;
                value_ce[r] = -logf(fminf(fmaxf(pt, CCE_EPS), CCE_HI));
                const float cv = w_v * inv_b;
                const float cvr = row_w != nullptr ? __fmul_rn(cv, wi) : cv;
#pragma unroll
                for (int k = 0; k < 3; ++k) grad_v[3 * r + k] = cvr * (p[k] * Sv - (k == tc ? Sv : 0.f));
            }
        } else if (lane == 0) {
            float t = z[i];
            if (q != nullptr) {                          // z/q mix (cz_policy_value_loss_q): rounded step by step, no fma
                const float qi = q[i];
                if (qi == qi) t = __fadd_rn(t, __fmul_rn(q_ratio, __fsub_rn(qi, t)));
            }
            const float d = v[r] - t;
            policy_loss[r] = loss;
            value_sqerr[r] = d * d;
            const float gv = w_v * (2.f * d) * inv_b;
            grad_v[r] = row_w != nullptr ? __fmul_rn(gv, wi) : gv;
        }
        wave_sync();
    }
}

// The moves-left output's loss (cz_moves_left_loss): one thread per minibatch row, nothing shared between rows.  x is the
// head's raw output; its meaning is unit * softplus(x) plies, so the loss is taken in units: Huber of softplus(x) - left / unit.
__global__ __launch_bounds__(256) void k_moves_left_loss(
    const float* __restrict__ x, const int32_t* __restrict__ idx, int n_rows, int n_pos, const int32_t* __restrict__ left,
    const float* __restrict__ row_w, float unit, float delta, float w_m, float* __restrict__ loss, float* __restrict__ grad_x)
{
    const float c = w_m * (1.0f / (float)n_rows);
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += gridDim.x * blockDim.x) {
        const int i = idx[r];
        if (i < 0 || i >= n_pos) {                       // out-of-range index: zero loss and gradient, nothing read
            loss[r] = 0.f;
            grad_x[r] = 0.f;
            continue;
        }
        const float xr = x[r];
        const float en = expf(-fabsf(xr));               // in (0, 1]: neither form below can overflow
        const float y = fmaxf(xr, 0.f) + log1pf(en);     // softplus(x)
        const float sg = xr >= 0.f ? 1.f / (1.f + en) : en / (1.f + en);      // sigmoid(x) = d softplus / dx
        const float d = y - (float)left[i] / unit;
        const float ad = fabsf(d);
        loss[r] = ad <= delta ? 0.5f * d * d : delta * (ad - 0.5f * delta);
        const float cr = row_w != nullptr ? __fmul_rn(c, row_w[i]) : c;
        grad_x[r] = cr * (fminf(fmaxf(d, -delta), delta) * sg);
    }
}

// ---- C-ABI ----------------------------------------------------------------------------
extern "C" {

int cz_moves_left_loss(const float* x, const int32_t* idx, int n_rows, int n_pos, const int32_t* left, const float* row_w,
                       float unit, float delta, float w_m, float* loss, float* grad_x, void* stream)
{
    if (n_rows == 0) return CZ_OK;
    if (n_rows < 0 || n_pos < 0 || !x || !idx || !loss || !grad_x || (n_pos > 0 && !left) || !(unit > 0.f) || !(delta > 0.f) ||
        !(unit < INFINITY) || !(delta < INFINITY) || !(w_m >= 0.f) || !(w_m < INFINITY)) {
        czi_set_error("cz_moves_left_loss: bad argument (unit and delta positive and finite, w_m >= 0 and finite)");
        return CZ_ERR_ARG;
    }
    const int blocks = (n_rows + 255) / 256;
    hipLaunchKernelGGL(k_moves_left_loss, dim3(blocks < 1024 ? blocks : 1024), dim3(256), 0, (hipStream_t)stream, x, idx, n_rows,
                       n_pos, left, row_w, unit, delta, w_m, loss, grad_x);
    return launch_status("cz_moves_left_loss: launch failed");
}

int cz_replay_games(const int8_t* init_boards, const uint16_t* labels, const int32_t* offsets, int n_games, int n_pos,
                    int8_t* boards, int32_t* prev, int32_t* bad_ply, void* stream)
{
    if (n_games == 0) return CZ_OK;
    if (n_games < 0 || n_pos < 0 || !init_boards || !offsets || !bad_ply || (n_pos > 0 && (!labels || !boards || !prev))) {
        czi_set_error("cz_replay_games: bad argument");
        return CZ_ERR_ARG;
    }
    hipLaunchKernelGGL(k_replay_games, dim3(grid_for(n_games)), dim3(64), 0, (hipStream_t)stream, init_boards, labels,
                       offsets, n_games, n_pos, boards, prev, bad_ply);
    return launch_status("cz_replay_games: launch failed");
}

int cz_gather_planes_m(const int8_t* boards, const int32_t* prev, int n_pos, const int32_t* idx, const uint8_t* mirror,
                       int n_rows, int depth, float* planes, void* stream)
{
    if (n_rows == 0) return CZ_OK;
    if (n_rows < 0 || n_pos < 0 || (depth != 14 && depth != 28) || !idx || !planes || (n_pos > 0 && !boards) ||
        (depth == 28 && n_pos > 0 && !prev)) {
        czi_set_error("cz_gather_planes: bad argument (depth 14 or 28)");
        return CZ_ERR_ARG;
    }
    hipLaunchKernelGGL(k_gather_planes, dim3(grid_for(n_rows)), dim3(64), 0, (hipStream_t)stream, boards, prev, n_pos, idx,
                       mirror, n_rows, depth, planes);
    return launch_status("cz_gather_planes: launch failed");
}

int cz_gather_planes(const int8_t* boards, const int32_t* prev, int n_pos, const int32_t* idx, int n_rows, int depth,
                     float* planes, void* stream)
{
    return cz_gather_planes_m(boards, prev, n_pos, idx, nullptr, n_rows, depth, planes, stream);
}

}  // extern "C"

namespace {

// cz_policy_value_loss_w and cz_policy_value_loss_l: one argument check, and the kernel with or without the legal-move mask
// (likewise cz_policy_wdl_loss and cz_policy_wdl_loss_l below)
template <bool MASK>
int launch_value_loss(const float* logits, int ld, const float* v, const int32_t* idx, const uint8_t* mirror, int n_rows,
                      int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                      const uint16_t* played, const float* z, const float* q, float q_ratio, const float* row_w, int mode,
                      float w_p, float w_v, float* policy_loss, float* value_sqerr, float* grad_logits, float* grad_v,
                      const int8_t* boards, int32_t* off_mask, float* illegal_mass, float* illegal_margin, void* stream)
{
    if (MASK && !boards) {
        czi_set_error("cz_policy_value_loss_l: boards is NULL");
        return CZ_ERR_ARG;
    }
    if (!(q_ratio >= 0.f && q_ratio <= 1.f)) {
        czi_set_error("cz_policy_value_loss_q: q_ratio outside [0, 1]");
        return CZ_ERR_ARG;
    }
    if (n_rows == 0) return CZ_OK;
    if (q_ratio == 0.f) q = nullptr;                     // the kernel's own test: no q, the target is z
    if (n_rows < 0 || n_pos < 0 || ld < CZ_NLABELS || (mode != 0 && mode != 1) || !logits || !v || !idx || !policy_loss ||
        !value_sqerr || !grad_logits || !grad_v || (n_pos > 0 && (!played || !z)) ||
        nnz < 0 || (mode == 1 && nnz > 0 && (!row_ptr || !vis_label || !vis_count))) {
        czi_set_error("cz_policy_value_loss: bad argument (ld >= 2086, mode 0 played / 1 visits)");
        return CZ_ERR_ARG;
    }
    hipLaunchKernelGGL((k_policy_value_loss<false, MASK>), dim3(grid_for(n_rows)), dim3(64), 0, (hipStream_t)stream, logits, ld,
                       v, idx, mirror, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z, q, q_ratio, row_w, mode,
                       w_p, w_v, policy_loss, value_sqerr, grad_logits, grad_v, (float*)nullptr, boards, off_mask,
                       illegal_mass, illegal_margin);
    return launch_status("cz_policy_value_loss: launch failed");
}

template <bool MASK>
int launch_wdl_loss(const float* logits, int ld, const float* vlogits, const int32_t* idx, const uint8_t* mirror, int n_rows,
                    int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                    const uint16_t* played, const float* z, const float* row_w, int mode, float w_p, float w_v,
                    float* policy_loss, float* value_ce, float* value_sqerr, float* grad_logits, float* grad_vlogits,
                    const int8_t* boards, int32_t* off_mask, float* illegal_mass, float* illegal_margin, void* stream)
{
    if (MASK && !boards) {
        czi_set_error("cz_policy_wdl_loss_l: boards is NULL");
        return CZ_ERR_ARG;
    }
    if (n_rows == 0) return CZ_OK;
    if (n_rows < 0 || n_pos < 0 || ld < CZ_NLABELS || (mode != 0 && mode != 1) || !logits || !vlogits || !idx || !policy_loss ||
        !value_ce || !value_sqerr || !grad_logits || !grad_vlogits || (n_pos > 0 && (!played || !z)) ||
        nnz < 0 || (mode == 1 && nnz > 0 && (!row_ptr || !vis_label || !vis_count))) {
        czi_set_error("cz_policy_wdl_loss: bad argument (ld >= 2086, mode 0 played / 1 visits)");
        return CZ_ERR_ARG;
    }
    hipLaunchKernelGGL((k_policy_value_loss<true, MASK>), dim3(grid_for(n_rows)), dim3(64), 0, (hipStream_t)stream, logits, ld,
                       vlogits, idx, mirror, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z, (const float*)nullptr,
                       0.f, row_w, mode, w_p, w_v, policy_loss, value_sqerr, grad_logits, grad_vlogits, value_ce, boards,
                       off_mask, illegal_mass, illegal_margin);
    return launch_status("cz_policy_wdl_loss: launch failed");
}

}  // namespace

extern "C" {

int cz_policy_value_loss_w(const float* logits, int ld, const float* v, const int32_t* idx, const uint8_t* mirror, int n_rows,
                           int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                           const uint16_t* played, const float* z, const float* q, float q_ratio, const float* row_w, int mode,
                           float w_p, float w_v, float* policy_loss, float* value_sqerr, float* grad_logits, float* grad_v,
                           void* stream)
{
    return launch_value_loss<false>(logits, ld, v, idx, mirror, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z, q,
                                    q_ratio, row_w, mode, w_p, w_v, policy_loss, value_sqerr, grad_logits, grad_v, nullptr,
                                    nullptr, nullptr, nullptr, stream);
}

int cz_policy_value_loss_l(const float* logits, int ld, const float* v, const int32_t* idx, const uint8_t* mirror, int n_rows,
                           int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                           const uint16_t* played, const float* z, const float* q, float q_ratio, const float* row_w, int mode,
                           float w_p, float w_v, float* policy_loss, float* value_sqerr, float* grad_logits, float* grad_v,
                           const int8_t* boards, int32_t* off_mask, float* illegal_mass, float* illegal_margin, void* stream)
{
    return launch_value_loss<true>(logits, ld, v, idx, mirror, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z, q,
                                   q_ratio, row_w, mode, w_p, w_v, policy_loss, value_sqerr, grad_logits, grad_v, boards,
                                   off_mask, illegal_mass, illegal_margin, stream);
}

int cz_policy_wdl_loss(const float* logits, int ld, const float* vlogits, const int32_t* idx, const uint8_t* mirror, int n_rows,
                       int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                       const uint16_t* played, const float* z, const float* row_w, int mode, float w_p, float w_v,
                       float* policy_loss, float* value_ce, float* value_sqerr, float* grad_logits, float* grad_vlogits,
                       void* stream)
{
    return launch_wdl_loss<false>(logits, ld, vlogits, idx, mirror, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z,
                                  row_w, mode, w_p, w_v, policy_loss, value_ce, value_sqerr, grad_logits, grad_vlogits, nullptr,
                                  nullptr, nullptr, nullptr, stream);
}

int cz_policy_wdl_loss_l(const float* logits, int ld, const float* vlogits, const int32_t* idx, const uint8_t* mirror, int n_rows,
                         int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                         const uint16_t* played, const float* z, const float* row_w, int mode, float w_p, float w_v,
                         float* policy_loss, float* value_ce, float* value_sqerr, float* grad_logits, float* grad_vlogits,
                         const int8_t* boards, int32_t* off_mask, float* illegal_mass, float* illegal_margin, void* stream)
{
    return launch_wdl_loss<true>(logits, ld, vlogits, idx, mirror, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z,
                                 row_w, mode, w_p, w_v, policy_loss, value_ce, value_sqerr, grad_logits, grad_vlogits, boards,
                                 off_mask, illegal_mass, illegal_margin, stream);
}

int cz_policy_value_loss_q(const float* logits, int ld, const float* v, const int32_t* idx, const uint8_t* mirror, int n_rows,
                           int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                           const uint16_t* played, const float* z, const float* q, float q_ratio, int mode, float w_p,
                           float w_v, float* policy_loss, float* value_sqerr, float* grad_logits, float* grad_v,
                           void* stream)
{
    return cz_policy_value_loss_w(logits, ld, v, idx, mirror, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z,
                                  q, q_ratio, nullptr, mode, w_p, w_v, policy_loss, value_sqerr, grad_logits, grad_v,
                                  stream);
}

int cz_policy_value_loss_m(const float* logits, int ld, const float* v, const int32_t* idx, const uint8_t* mirror, int n_rows,
                           int n_pos, const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                           const uint16_t* played, const float* z, int mode, float w_p, float w_v, float* policy_loss,
                           float* value_sqerr, float* grad_logits, float* grad_v, void* stream)
{
    return cz_policy_value_loss_q(logits, ld, v, idx, mirror, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z,
                                  nullptr, 0.f, mode, w_p, w_v, policy_loss, value_sqerr, grad_logits, grad_v, stream);
}

int cz_policy_value_loss(const float* logits, int ld, const float* v, const int32_t* idx, int n_rows, int n_pos,
                         const int32_t* row_ptr, const uint16_t* vis_label, const int32_t* vis_count, int nnz,
                         const uint16_t* played, const float* z, int mode, float w_p, float w_v, float* policy_loss,
                         float* value_sqerr, float* grad_logits, float* grad_v, void* stream)
{
    return cz_policy_value_loss_m(logits, ld, v, idx, nullptr, n_rows, n_pos, row_ptr, vis_label, vis_count, nnz, played, z,
                                  mode, w_p, w_v, policy_loss, value_sqerr, grad_logits, grad_v, stream);
}

// HOST table of the label mirror M, from the same two tables the device path reads.
int cz_label_mirror(uint16_t* out)
{
    if (!out) {
        czi_set_error("cz_label_mirror: bad argument");
        return CZ_ERR_ARG;
    }
    for (int l = 0; l < NLABELS; ++l) {
        const int ft = h_tab.lab_ft[l];
        const int f = ft >> 8, t = ft & 0xFF;
        out[l] = h_tab.label_of[(f + 8 - 2 * (f % 9)) * NSQ + (t + 8 - 2 * (t % 9))];
    }
    return CZ_OK;
}

}  // extern "C"
