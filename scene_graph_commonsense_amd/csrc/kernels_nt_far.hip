// The far-tile pass of the listed-window NT block (gemm_nt_pp_far_kernel, csrc/gemm_nt_pp.h), instantiated apart from the kernels it follows.
#include "gemm_nt.h"

template <int ELEM, int EPI>
static int launch_far(const NtParams& p, int lds, hipStream_t stream) {
    auto kern = gemm_nt_pp_far_kernel<ELEM, EPI>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    SGC_LAUNCH(kern, dim3((unsigned)((p.tiles_m + 7) / 8)), dim3(512), lds, stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

int sgc_nt_pp_far_launch(int elem, int epi, const NtParams& p, int lds, hipStream_t stream) {
    if (elem != ELEM_F16) return SGC_ERR_ARG;                  // the listed-window launches of the library: conv3 pool / raw, conv2 regions
    if (epi == EPI_POOL) return launch_far<ELEM_F16, EPI_POOL>(p, lds, stream);
    if (epi == EPI_STORE) return launch_far<ELEM_F16, EPI_STORE>(p, lds, stream);
    if (epi == EPI_STORE_F32) return launch_far<ELEM_F16, EPI_STORE_F32>(p, lds, stream);
    return SGC_ERR_ARG;
}
