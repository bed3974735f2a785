// xq_conv_ip4.hip -- the 128-filter chains of the c8 / c6 tower on the four-wave pair kernel (k_resblock_ip4_c8<128>,
// csrc/xq_conv_ip4.h), in a translation unit of their own: build.py compiles this file, and no other, with
// -mllvm -amdgpu-mfma-vgpr-form.  The compiler then keeps a wave's 96 accumulators in ordinary VGPRs, which the epilogues'
// VALU instructions read and write directly, instead of in AGPRs behind v_accvgpr_read / v_accvgpr_write (the kernel runs one
// 512-register wave per SIMD: between the K loops its time is its instruction count).  The 192-filter instantiations stay in
// csrc/xq_conv.hip: with the option the chain that starts a 192-filter tower spills more.  EXPERIMENTS.md has the figures.
#define CZ_IP4_VGPR_FORM 1
#include "xq_conv_ip4.h"

#ifdef CZ_IP4_STAMPS
extern "C" int cz_debug_ip4_stamps(long long* out384_host)
{
    return hipMemcpyFromSymbol(out384_host, HIP_SYMBOL(g_ip4_stamps), sizeof(g_ip4_stamps)) == hipSuccess ? CZ_OK : CZ_ERR_HIP;
}
#endif

// cz_tower's launches on the four-wave kernel (csrc/xq_nn_launch.h)
extern "C" int czi_tower4_launch(const char* name, const void* x_hi, const void* x_img, const BlockChain<12>* ch, int c6,
                                 int exit_mode, void* y_hi, void* y_img, const float* head_w, const float* head_b, float* pol,
                                 float* val, int n_pol, int n_boards, int n_cu, const int32_t* n_dev, void* stream)
{
    const HeadArgs hd{head_w, head_b, pol, val, n_pol};
    const ChainCall a{x_hi, x_img, *ch, y_hi, y_img, nullptr, n_boards, n_cu, n_dev, (hipStream_t)stream};
    if (c6) launch_ip4<128, 1, 1>(a, exit_mode, hd);
    else launch_ip4<128, 0, 0>(a, exit_mode, hd);
    return nn_launched(name);
}
