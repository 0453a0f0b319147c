// env_push_block.hip -- the kernels of rollout_episodes.h for the push-block environment (PushBlockEnvDev, env_device.h), and the
// two launchers the dispatches of rollout.hip call for HP_ENV_PUSH_BLOCK.  A unit of its own so that rollout.hip keeps compiling
// exactly one instantiation of k_rollout_episodes (the policy slab's body is the bulk of either unit's compile).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-inline"   // agent_device.h declares the 32-row engine's fragment map, which no code here calls
#include "agent_device.h"
#pragma clang diagnostic pop

// the 4-row policy slab's device functions (no kernel of slab8.h is compiled here)
#define S8_DEVICE_ONLY
#define S8_NRG 1
#define S8_NS s8ro
#include "slab8.h"
#undef S8_NRG
#undef S8_NS
#undef S8_DEVICE_ONLY

#include "rollout_episodes.h"

static_assert(PushBlockEnvDev::ACT <= 4 && PushBlockEnvDev::OBS + PushBlockEnvDev::GOAL <= S8_LDX, "an environment of the policy slab's shape");
static_assert(PushBlockEnvDev::RESET_DRAWS <= RO_MAX_ACT, "the reset's values pass through the row's zs");

hipError_t push_block_launch_episodes(hipStream_t stream, unsigned blocks, const EpisodesArgs &L) {
    hipLaunchKernelGGL(k_rollout_episodes<PushBlockEnvDev>, dim3(blocks), dim3(S8_THREADS), 0, stream, L);
    return hipGetLastError();
}

hipError_t push_block_launch_reset(hipStream_t stream, const hp_env_desc &env, MtState *reset_st, int64_t rows) {
    hipLaunchKernelGGL(k_env_reset<PushBlockEnvDev>, dim3((unsigned)rows), dim3(MW_THREADS), 0, stream, env, reset_st);
    return hipGetLastError();
}
