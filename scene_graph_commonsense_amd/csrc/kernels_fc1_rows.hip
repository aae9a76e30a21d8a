// fc1 backward over the compact window-major rows WITHOUT the window-major gradient buffer (csrc/kernels_shared.hip: "fc1 over shared
// windows"): both grouped GEMMs read their gradient rows where they lie, through the row table of sgc_window_rows_source, from
//     gsrc [gsrc_rows][4096] bf16 = [the rows of dh1][one zero row][the per-object sums of sgc_fc1_gsum_compact, group after group].
// A pair's row of dh1 stands in about seven window groups: the copy path (sgc_fc1_xrows + sgc_fc1_windows_dgrad / _wgrad) wrote it seven
// times and each GEMM read the seven copies back; here nothing is written and the GEMMs re-read one tensor of a few hundred MB.  Every A
// value and every K position is where it was: the same bits as the copy path (tests/test_fc1_rows_gather_gpu.py).
// Range: both blocks address A by 32-bit per-lane byte offsets from gsrc under one buffer descriptor; a load past 2 GiB returns zeros
// without a fault, so a source of more than 262144 rows is refused here and the engine keeps the copy path for it.
// The instantiations live in this translation unit so that the kernels next to the plain entries compile as they did.
#include "gemm_nt.h"
#include "gemm_tn.h"

constexpr int FC1_ROWS_LIMIT = 262144;       // rows of 8 KiB in 2 GiB

extern "C" {

// dywm [rows][1024] bf16 = gsrc[rowsrc[.]] * (rows g*1024.. of w1pT [65536][4096])^T, g = tile_group[row / 256]; every rowsrc[r] < gsrc_rows
int sgc_fc1_windows_dgrad_rows(const void* gsrc, const int* rowsrc, int gsrc_rows, const void* w1pT, const int* tile_group, void* dywm,
                               int rows, void* stream) {
    if (rows <= 0) return SGC_OK;
    if ((rows & 255) || !rowsrc || gsrc_rows <= 0 || gsrc_rows > FC1_ROWS_LIMIT) return SGC_ERR_ARG;
    NtParams p{};
    p.A = (const u16*)gsrc; p.B = (const u16*)w1pT; p.C = dywm; p.M = rows; p.N = 1024; p.K = 4096;
    p.lda = 4096; p.ldb = 4096; p.ldc = 1024; p.tile_group = tile_group; p.group_stride = 1024L * 4096;
    p.gather = rowsrc;
    p.epi_lds = 1;
    return launch_gemm_nt_pp_rows<ELEM_BF16, EPI_STORE>(p, (hipStream_t)stream);
}

// dw [4096][65536] f32 (columns in (window, channel) order): block g = gsrc[rowsrc[group g]]^T * ywm_bf16[group g]
int sgc_fc1_windows_wgrad_rows(const void* gsrc, const int* rowsrc, int gsrc_rows, const void* ywm_bf16, const int* goff, float* dw, int rows,
                               void* stream) {
    if (rows <= 0) return SGC_OK;
    if ((rows & 63) || !rowsrc || !goff || gsrc_rows <= 0 || gsrc_rows > FC1_ROWS_LIMIT || ((uintptr_t)rowsrc & 15)) return SGC_ERR_ARG;
    TnParams p{};
    p.A = (const u16*)gsrc; p.B = (const u16*)ywm_bf16; p.C = dw; p.M = 4096; p.N = 1024; p.K = rows;
    p.lda = 4096; p.ldb = 1024; p.ldc = 65536; p.goff = goff;
    p.gather = rowsrc;
    p.tiles_m = 16; p.tiles_n = 4; p.ktiles_per_split = 0; p.splits = 64; p.xcd_map = 0; p.xcd_patch = 1;
    auto kern = gemm_tn_pp_rows_kernel<ELEM_BF16>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 8 * 16384);
    SGC_LAUNCH(kern, dim3(64 * 64), dim3(512), 8 * 16384, (hipStream_t)stream, p);
    SGC_CHECK_LAUNCH();
    return SGC_OK;
}

}  // extern "C"
