// forward_kernels.h -- the four pack kernels of the layer-per-launch forward chain (mlp_rows, agent_forward.hip): declared for the
// unit that launches them, defined (FORWARD_KERNELS_HERE) in the unit that compiles them, agent_engines.hip, behind k_polyak_frag.
// They are compiled there, at the place they always had, because the code object's layout is measured: the k_fb_split8
// instantiations are emitted behind the last kernel of that unit, and with these four gone from in front of them the benchmark's
// update ran 0.9 % slower on identical instructions (profiles/policy_call_refactor.txt, section 4).
#pragma once
#include "transition_device.h"

__global__ void k_pack_inputs(const float *__restrict__ src, int rows, int width, float *dst, int ld, int col0);
__global__ void k_policy_inputs(const double *__restrict__ obs, const double *__restrict__ g, int rows, int od, int gd,
                                const NormDev *__restrict__ onz, const NormDev *__restrict__ gnz, double clip_obs,
                                double clip_o, double clip_g, float *X, int ld);
__global__ void k_pack_scaled_actions(const float *__restrict__ src, int rows, int act_dim, float *dst, int ld, int act_off,
                                      float max_action);
__global__ void k_unpack_actions(const float *__restrict__ X, int rows, int ld, int act_off, int act_dim, float max_action,
                                 float *out);

#ifdef FORWARD_KERNELS_HERE
// layer engine: float32 rows [rows][width] -> columns col0.. of the padded input rows
__global__ void k_pack_inputs(const float *__restrict__ src, int rows, int width, float *dst, int ld, int col0) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * width) return;
    const int r = idx / width, c = idx - r * width;
    dst[(long long)r * ld + col0 + c] = src[idx];
}

// rollout inputs (ddpg_agent._preproc_inputs :163-171): normalised, clipped observation | goal rows in float32 (tr_net_input)
__global__ void k_policy_inputs(const double *__restrict__ obs, const double *__restrict__ g, int rows, int od, int gd,
                                const NormDev *__restrict__ onz, const NormDev *__restrict__ gnz, double clip_obs,
                                double clip_o, double clip_g, float *X, int ld) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int w = od + gd;
    if (idx >= (long long)rows * w) return;
    const int r = (int)(idx / w), c = (int)(idx - (long long)r * w);
    const int j = c - od;
    X[(long long)r * ld + c] = c < od ? tr_net_input(obs[(long long)r * od + c], clip_obs, onz->mean[c], onz->std[c], clip_o)
                                      : tr_net_input(g[(long long)r * gd + j], clip_obs, gnz->mean[j], gnz->std[j], clip_g);
}

// critic input: action block = actions / max_action (models.py:38)
__global__ void k_pack_scaled_actions(const float *__restrict__ src, int rows, int act_dim, float *dst, int ld, int act_off,
                                      float max_action) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * act_dim) return;
    const int r = idx / act_dim, c = idx - r * act_dim;
    dst[(long long)r * ld + act_off + c] = src[idx] / max_action;
}

__global__ void k_unpack_actions(const float *__restrict__ X, int rows, int ld, int act_off, int act_dim,
                                 float max_action, float *out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * act_dim) return;
    const int r = idx / act_dim, c = idx - r * act_dim;
    out[idx] = X[(long long)r * ld + act_off + c] * max_action;   // stored value is actions / max_action
}
#endif  // FORWARD_KERNELS_HERE
