// demo_compact.hip -- the success filter of the scripted demonstrations (hp_demo_compact, rollout.hip): order-preserving
// compaction of a round's successful episodes behind those kept so far.
#include "demo_episodes.h"

// hp_demo_compact.  Workgroup e looks at episode e of the round: its rank among the round's successes is the count of flags in
// front of it, which the workgroup sums itself -- a round is a few thousand flags, so each of the few workgroups that have
// anything to copy reads them once, and nothing is handed from one workgroup to another.  Workgroup 0 counts the whole round
// and writes the new total.  Order is preserved by construction: slot = kept + rank.
__global__ __launch_bounds__(256) void k_demo_compact(const CompactArgs A) {
    __shared__ int count;
    const int e = blockIdx.x, tid = threadIdx.x;
    const int lim = e == 0 ? A.n : e;            // workgroup 0: the round's total (its own rank is 0)
    if (tid == 0) count = 0;
    __syncthreads();
    int c = 0;
    for (int k = tid; k < lim; k += 256) c += A.success[k] != 0.f ? 1 : 0;
    if (c) atomicAdd(&count, c);
    __syncthreads();
    const int total = count;
    if (e == 0 && tid == 0) *A.kept_out = (int)(A.kept + total < A.n_demos ? A.kept + total : A.n_demos);
    const long long slot = A.kept + (e == 0 ? 0 : total);
    if (A.success[e] == 0.f || slot >= A.n_demos) return;
    const long long T = A.T, n_o = (T + 1) * A.od, n_ag = (T + 1) * A.gd, n_g = T * A.gd, n_a = T * A.ad;
    for (long long k = tid; k < n_o; k += 256) A.d_obs[slot * n_o + k] = A.s_obs[e * n_o + k];
    for (long long k = tid; k < n_ag; k += 256) A.d_ag[slot * n_ag + k] = A.s_ag[e * n_ag + k];
    for (long long k = tid; k < n_g; k += 256) A.d_g[slot * n_g + k] = A.s_g[e * n_g + k];
    for (long long k = tid; k < n_a; k += 256) A.d_act[slot * n_a + k] = A.s_act[e * n_a + k];
    for (long long k = tid; k < T; k += 256) A.d_step[slot * T + k] = A.s_step[e * T + k];
}

hipError_t demo_launch_compact(hipStream_t stream, unsigned episodes, const CompactArgs &A) {
    hipLaunchKernelGGL(k_demo_compact, dim3(episodes), dim3(256), 0, stream, A);
    return hipGetLastError();
}
