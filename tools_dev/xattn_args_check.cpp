// Host-side check of csrc/xattn.hip's launchers: argument validation and the workspace-size query are pure
// host logic that returns before any device work, so this program needs no GPU. Built with the host sanitizers:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       tools_dev/xattn_args_check.cpp vfm-vae_amd/csrc/xattn.hip vfm-vae_amd/csrc/version.hip -o xattn_args_check
//   ./xattn_args_check
#include <cstdio>
#include <cstdlib>

#include "../include/vfmvae.h"

static int failures = 0;
#define EXPECT(expr, want)                                                                      \
    do {                                                                                        \
        const long long got_ = (long long)(expr);                                               \
        if (got_ != (long long)(want)) {                                                        \
            std::printf("FAIL %s = %lld, expected %lld\n", #expr, got_, (long long)(want));      \
            ++failures;                                                                         \
        }                                                                                       \
    } while (0)

int main() {
    alignas(16) static float buf[64];
    void* p = buf;
    void* odd = (char*)buf + 4;                      // not 16-B aligned
    const long long s4[3] = {4096, 64, 64}, s3[3] = {4096, 63, 64}, s8[3] = {4096, 64, 64}, s7[3] = {4096, 60, 64};

    // workspace query: delta [B H Nq] (rounded to 4) + chunks x [B, H, L + 1, 2, d]
    EXPECT(vfm_cross_attention_f32_workspace_floats(32, 8, 1024, 64, 64), 262144 + 1LL * 32 * 8 * 65 * 2 * 64);
    EXPECT(vfm_cross_attention_f32_workspace_floats(2, 2, 160, 64, 64), 640 + 3LL * 2 * 2 * 65 * 2 * 64);
    EXPECT(vfm_cross_attention_f32_workspace_floats(1, 1, 1, 1, 32), 4 + 1LL * 2 * 2 * 32);
    EXPECT(vfm_cross_attention_f32_workspace_floats(65535, 65535, 1 << 30, 127, 64) > 0, 1);     // no int overflow
    EXPECT(vfm_cross_attention_f32_workspace_floats(65535, 65535, 2147483647, 127, 64), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_workspace_floats(2, 2, 64, 2147483647, 64), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_workspace_floats(0, 8, 64, 64, 64), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_workspace_floats(2, 70000, 64, 64, 64), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_workspace_floats(2, 2, -5, 64, 64), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_workspace_floats(2, 2, 64, 0, 64), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_workspace_floats(2, 2, 64, 128, 64), VFM_NO_KERNEL);
    EXPECT(vfm_cross_attention_f32_workspace_floats(2, 2, 64, 64, 48), VFM_NO_KERNEL);

    // forward
    EXPECT(vfm_cross_attention_f32_fwd(nullptr, p, p, nullptr, p, p, 2, 2, 64, 64, 64, s4, s4, 0.125f, 0, VFM_F32, nullptr),
           VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_fwd(p, p, p, nullptr, p, nullptr, 2, 2, 64, 64, 64, s4, s4, 0.125f, 0, VFM_F32, nullptr),
           VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_fwd(p, p, p, nullptr, p, p, 2, 2, 64, 64, 64, nullptr, s4, 0.125f, 0, VFM_F32, nullptr),
           VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_fwd(p, p, p, nullptr, p, p, 2, 2, 64, 64, 64, s3, s4, 0.125f, 0, VFM_F32, nullptr),
           VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_fwd(p, odd, p, nullptr, p, p, 2, 2, 64, 64, 64, s4, s4, 0.125f, 0, VFM_F32, nullptr),
           VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_fwd(p, p, p, nullptr, p, p, 2, 2, 64, 64, 64, s4, s4, 0.125f, 0, VFM_BF16, nullptr),
           VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_fwd(p, p, p, nullptr, p, p, 2, 2, 0, 64, 64, s4, s4, 0.125f, 0, VFM_F32, nullptr),
           VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_fwd(p, p, p, nullptr, p, p, 2, 2, 64, 128, 64, s4, s4, 0.125f, 0, VFM_F32, nullptr),
           VFM_NO_KERNEL);
    EXPECT(vfm_cross_attention_f32_fwd(p, p, p, nullptr, p, p, 2, 2, 64, 64, 128, s4, s4, 0.125f, 0, VFM_F32, nullptr),
           VFM_NO_KERNEL);

    // backward
    EXPECT(vfm_cross_attention_f32_bwd(p, p, p, nullptr, p, p, p, nullptr, p, p, p, 2, 2, 64, 64, 64, s4, s4, s4, s4, 0.125f,
                                       0, VFM_F32, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_bwd(p, p, p, nullptr, p, p, p, p, p, p, nullptr, 2, 2, 64, 64, 64, s4, s4, s4, s4, 0.125f,
                                       1, VFM_F32X3, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_bwd(p, p, p, nullptr, p, p, p, p, p, p, p, 2, 2, 64, 64, 64, s4, s4, nullptr, s4, 0.125f,
                                       0, VFM_F32, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_bwd(p, p, p, nullptr, p, p, p, odd, p, p, p, 2, 2, 64, 64, 64, s4, s4, s4, s4, 0.125f, 0,
                                       VFM_F32, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_bwd(p, p, p, nullptr, p, p, p, p, p, p, p, 2, 2, 64, 64, 64, s4, s4, s4, s3, 0.125f, 0,
                                       VFM_F32, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_cross_attention_f32_bwd(p, p, p, nullptr, p, p, p, p, p, p, p, 2, 2, 64, 200, 32, s4, s4, s4, s4, 0.125f, 0,
                                       VFM_F32, nullptr), VFM_NO_KERNEL);

    // the text tower's key-masked attention
    EXPECT(vfm_attention_keymask_fwd(nullptr, p, p, nullptr, p, 2, 2, 64, 64, s8, s8, s8, s8, 0.125f, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_attention_keymask_fwd(p, p, p, nullptr, p, 2, 2, 64, 64, s8, s7, s8, s8, 0.125f, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_attention_keymask_fwd(p, p, p, nullptr, p, 2, 2, 64, 64, s8, s8, s8, nullptr, 0.125f, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_attention_keymask_fwd(p, p, odd, nullptr, p, 2, 2, 64, 64, s8, s8, s8, s8, 0.125f, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_attention_keymask_fwd(p, p, p, nullptr, p, 2, 2, 0, 64, s8, s8, s8, s8, 0.125f, nullptr), VFM_ERR_ARGS);
    EXPECT(vfm_attention_keymask_fwd(p, p, p, nullptr, p, 2, 2, 129, 64, s8, s8, s8, s8, 0.125f, nullptr), VFM_NO_KERNEL);
    EXPECT(vfm_attention_keymask_fwd(p, p, p, nullptr, p, 2, 2, 64, 80, s8, s8, s8, s8, 0.125f, nullptr), VFM_NO_KERNEL);

    std::printf(failures ? "%d check(s) failed\n" : "xattn argument checks ok\n", failures);
    return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
