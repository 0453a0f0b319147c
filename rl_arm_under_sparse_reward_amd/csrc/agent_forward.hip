// agent_forward.hip -- the rollout-side forward: the policy calls (hp_agent_act, hp_agent_act_dev, hp_agent_actor_forward,
// hp_agent_act_snapshot behind hp_agent_policy_snapshot) and the stand-alone critic (hp_agent_critic_forward).  Host code only:
// the kernels it launches are compiled by agent_engines.hip (k_policy_slab8 in slab8.h, the four pack kernels in forward_kernels.h).
// Reference: ddpg_agent._preproc_inputs (:163-171), models.py:11-44.
//
// Two engines, as for an update.  The thin-slab engine answers a policy call with ONE launch, k_policy_slab8: a 4-row slab per
// workgroup through the actor half of the chain kernels (s8_policy_slab, slab8.h) -- the same device functions, so the same bits,
// as the training forward.  The kernel is compiled with the chain kernels, in agent_engines.hip (moved here it kept its registers,
// LDS and instruction count but not its instruction order: profiles/policy_call_refactor.txt), and launch_policy_slab there is the
// only place that launches it; staged_policy_call wraps it in the upload and the download of a call on host rows.  Every other
// network shape, and the stand-alone critic, runs the layer-per-launch GEMMs (gemm_lds.h through launch_group): one chain,
// mlp_rows, for both networks.  What a policy call is made of -- the parameter set, the normalizer views, the argument block, the
// shared refusals -- is policy_call.h's.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wundefined-inline"   // agent_device.h declares the 32-row engine's fragment map, which no code here calls
#include "agent_device.h"   // AdamFuse, which the split launch's argument block in slab8.h's shared section holds
#pragma clang diagnostic pop
#define S8_SHARED_ONLY   // PolicyArgs and what it is made of: the section of slab8.h outside every slab height's namespace
#include "slab8.h"
#undef S8_SHARED_ONLY
#include "forward_kernels.h"
#include "policy_call.h"

// ------------------------------------------------------------------------------- host side
// A policy call of the slab engine on host rows, enqueued on `stream` with `ws` as its staging: upload, the one launch, download.
// The inputs are float32 network inputs (f32_inputs: host_a alone, on.size = their width) or the float64 observation rows followed
// by the goal rows.  Nothing waits here: the caller decides where
static int staged_policy_call(const hp_agent *a, DevBuf &ws, hipStream_t stream, const SlabNetPtrs &net, const NormView &on,
                              const NormView &gn, double clip_obs, int64_t rows, const void *host_a, const void *host_b,
                              bool f32_inputs, float *actions_host) {
    const int ad = a->cfg.act_dim;
    const size_t bytes_a = (size_t)rows * on.size * (f32_inputs ? 4 : 8), bytes_b = (size_t)rows * gn.size * 8;
    const size_t head = (bytes_a + bytes_b + 15) & ~(size_t)15;
    HP_TRY(ws.ensure(head + (size_t)rows * ad * 4));
    char *d = ws.as<char>();
    HP_CHECK_HIP(hipMemcpyAsync(d, host_a, bytes_a, hipMemcpyHostToDevice, stream));
    if (bytes_b) HP_CHECK_HIP(hipMemcpyAsync(d + bytes_a, host_b, bytes_b, hipMemcpyHostToDevice, stream));
    PolicyArgs P = policy_args(a, net, on, gn, clip_obs, rows);
    if (f32_inputs) {
        P.x = reinterpret_cast<const float *>(d);
    } else {
        P.obs = reinterpret_cast<const double *>(d);
        P.g = reinterpret_cast<const double *>(d + bytes_a);
    }
    P.actions = reinterpret_cast<float *>(d + head);
    HP_TRY(launch_policy_slab(stream, P));
    HP_CHECK_HIP(hipMemcpyAsync(actions_host, P.actions, (size_t)rows * ad * 4, hipMemcpyDeviceToHost, stream));
    return HP_OK;
}

// Rows through one network on the layer-per-launch GEMMs.  l / P: the network's layout and the base of its parameters; actor:
// the head is max_action * tanh over n_out actions (models.py:19-26), else the critic's plain n_out = 1 (models.py:28-44).
// Workspace: [head_bytes of caller data] | X rows | h1 | h2 | h3 | 16-wide head | out; `fill` enqueues whatever turns the
// caller data into X (zeroed beforehand).  out_dev: the outputs stay on the device, in stream order, no host wait (agent_act_dev);
// else they go to out_host and the call waits
template <typename Fill>
static int mlp_rows(hp_agent *a, const NetLayout &l, const float *P, bool actor, int n_out, int64_t rows, size_t head_bytes,
                    Fill fill, float *out_host, float *out_dev = nullptr) {
    const int H = a->H, ldx = a->ldx;
    const int Mp = roundup((int)rows, 32);
    hipStream_t s = a->ctx->stream;
    const size_t nX = (size_t)Mp * ldx, nH = (size_t)Mp * H, nT = (size_t)Mp * 16;
    head_bytes = (head_bytes + 15) & ~(size_t)15;
    HP_TRY(a->fwd_ws.ensure(head_bytes + (nX + 3 * nH + nT + (size_t)rows * n_out) * 4));
    char *head = a->fwd_ws.as<char>();
    float *X = reinterpret_cast<float *>(head + head_bytes), *h1 = X + nX, *h2 = h1 + nH, *h3 = h2 + nH, *y16 = h3 + nH,
          *outp = y16 + nT;
    HP_CHECK_HIP(hipMemsetAsync(X, 0, nX * 4, s));
    HP_TRY(fill(head, X, s));
    { Launch L; add_fwd(L, X, ldx, l.K1, P + l.w1, P + l.b1, h1, H, Mp, H, EPI_BIAS_RELU); HP_TRY(launch_group(a, L, PROF_GEMM_FWD)); }
    { Launch L; add_fwd(L, h1, H, H, P + l.w2, P + l.b2, h2, H, Mp, H, EPI_BIAS_RELU); HP_TRY(launch_group(a, L, PROF_GEMM_FWD)); }
    { Launch L; add_fwd(L, h2, H, H, P + l.w3, P + l.b3, h3, H, Mp, H, EPI_BIAS_RELU); HP_TRY(launch_group(a, L, PROF_GEMM_FWD)); }
    {
        Launch L;
        if (actor) {   // tanh into the action columns of X (where a critic would read it) and, 16 wide, into y16
            add_fwd(L, h3, H, H, P + l.w4, P + l.b4, X + a->act_off, ldx, Mp, 16, EPI_BIAS_TANH);
            L.g.p[0].C2 = y16; L.g.p[0].ldc2 = 16; L.g.p[0].max_action = (float)a->cfg.max_action;
        } else {
            add_fwd(L, h3, H, H, P + l.w4, P + l.b4, y16, 16, Mp, 16, EPI_BIAS);
        }
        L.g.p[0].n_store = n_out;
        HP_TRY(launch_group(a, L, PROF_GEMM_FWD));
    }
    // actions = max_action * tanh(.)  (models.py:24): y16 holds tanh; the critic's Q as it is
    hipLaunchKernelGGL(k_unpack_actions, dim3((unsigned)((rows * n_out + 255) / 256)), dim3(256), 0, s, y16, (int)rows, 16, 0, n_out,
                       actor ? (float)a->cfg.max_action : 1.0f, outp);
    HP_CHECK_HIP(hipGetLastError());
    if (out_dev) {
        HP_CHECK_HIP(hipMemcpyAsync(out_dev, outp, (size_t)rows * n_out * 4, hipMemcpyDeviceToDevice, s));
        return HP_OK;
    }
    HP_CHECK_HIP(hipMemcpyAsync(out_host, outp, (size_t)rows * n_out * 4, hipMemcpyDeviceToHost, s));
    HP_CHECK_HIP(hipStreamSynchronize(s));
    return HP_OK;
}

template <typename Fill>
static int actor_rows(hp_agent *a, int32_t net, int64_t rows, size_t head_bytes, float *actions_host, Fill fill,
                      float *actions_dev = nullptr) {
    return mlp_rows(a, a->la, net == HP_NET_ACTOR ? a->params : a->targets, true, a->cfg.act_dim, rows, head_bytes, fill,
                    actions_host, actions_dev);
}

// k_policy_inputs behind whatever put the float64 rows on the device: the fill of hp_agent_act and agent_act_dev
static int fill_policy_inputs(const hp_agent *a, const hp_norm *on, const hp_norm *gn, const double *obs_dev, const double *g_dev,
                              int64_t rows, double clip_obs, float *X, hipStream_t s) {
    const long long n = (long long)rows * (on->size + gn->size);
    hipLaunchKernelGGL(k_policy_inputs, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, obs_dev, g_dev, (int)rows, on->size,
                       gn->size, on->d, gn->d, clip_obs, on->clip, gn->clip, X, a->ldx);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// hp_agent_act for rows that already lie in device memory (a vectorised simulator's tensors, rollout.hip): the same kernels on the
// caller's pointers -- k_policy_slab8 reads obs / g and writes the actions in place, nothing is copied and nothing waits.
int agent_act_dev(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, const double *obs_dev, const double *g_dev, int64_t rows,
                  double clip_obs, float *actions_dev) {
    HP_TRY(check_policy_call("hp_agent_act_dev", a, on, gn, net, true, rows));
    const double co = clip_or_inf(clip_obs);
    if (a->slab8) {
        PolicyArgs P = policy_args(a, slab_net(a, net != HP_NET_ACTOR), norm_view(on), norm_view(gn), co, rows);
        P.obs = obs_dev; P.g = g_dev;
        P.actions = actions_dev;
        return launch_policy_slab(a->ctx->stream, P);
    }
    return actor_rows(a, net, rows, 0, nullptr, [&](char *, float *X, hipStream_t s) -> int {
        return fill_policy_inputs(a, on, gn, obs_dev, g_dev, rows, co, X, s);
    }, actions_dev);
}

extern "C" {

int hp_agent_act_dev(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, const double *obs_dev, const double *g_dev,
                     int64_t rows, double clip_obs, float *actions_dev) {
    HP_REQUIRE(a && on && gn && obs_dev && g_dev && actions_dev, HP_ERR_INVALID, "hp_agent_act_dev: null argument");
    HP_SERIALISE(a);
    return agent_act_dev(a, on, gn, net, obs_dev, g_dev, rows, clip_obs, actions_dev);
}

int hp_agent_actor_forward(hp_agent *a, int32_t net, const float *x_host, int64_t rows, float *actions_host) {
    HP_REQUIRE(a && x_host && actions_host, HP_ERR_INVALID, "hp_agent_actor_forward: null argument");
    HP_SERIALISE(a);
    HP_TRY(check_policy_call("hp_agent_actor_forward", a, nullptr, nullptr, net, true, rows));
    const int xd = a->xdim, ldx = a->ldx;
    const size_t n_raw = (size_t)rows * xd;
    if (a->slab8) {
        HP_TRY(staged_policy_call(a, a->fwd_ws, a->ctx->stream, slab_net(a, net != HP_NET_ACTOR), NormView{nullptr, 0.0, xd},
                                  NormView{nullptr, 0.0, 0}, 0.0, rows, x_host, nullptr, true, actions_host));
        HP_CHECK_HIP(hipStreamSynchronize(a->ctx->stream));
        return HP_OK;
    }
    return actor_rows(a, net, rows, n_raw * 4, actions_host, [&](char *head, float *X, hipStream_t s) -> int {
        float *raw = reinterpret_cast<float *>(head);
        HP_CHECK_HIP(hipMemcpyAsync(raw, x_host, n_raw * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_pack_inputs, dim3((unsigned)((n_raw + 255) / 256)), dim3(256), 0, s, raw, (int)rows, xd, X, ldx, 0);
        HP_CHECK_HIP(hipGetLastError());
        return (int)HP_OK;
    });
}

// stand-alone critic rows (models.py:28-44): Q(x, a) for host inputs, on the layer-per-launch GEMMs
int hp_agent_critic_forward(hp_agent *a, int32_t net, const float *x_host, const float *actions_host, int64_t rows,
                            float *q_host) {
    HP_REQUIRE(a && x_host && actions_host && q_host, HP_ERR_INVALID, "hp_agent_critic_forward: null argument");
    HP_SERIALISE(a);
    HP_TRY(check_policy_call("hp_agent_critic_forward", a, nullptr, nullptr, net, false, rows));
    const int xd = a->xdim, ad = a->cfg.act_dim, ldx = a->ldx;
    const size_t n_x = (size_t)rows * xd, n_a = (size_t)rows * ad;
    const float *P = (net == HP_NET_CRITIC ? a->params : a->targets) + a->la.total;
    return mlp_rows(a, a->lc, P, false, 1, rows, (n_x + n_a) * 4, [&](char *head, float *X, hipStream_t s) -> int {
        float *raw_x = reinterpret_cast<float *>(head), *raw_a = raw_x + n_x;
        HP_CHECK_HIP(hipMemcpyAsync(raw_x, x_host, n_x * 4, hipMemcpyHostToDevice, s));
        HP_CHECK_HIP(hipMemcpyAsync(raw_a, actions_host, n_a * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_pack_inputs, dim3((unsigned)((n_x + 255) / 256)), dim3(256), 0, s, raw_x, (int)rows, xd, X, ldx, 0);
        hipLaunchKernelGGL(k_pack_scaled_actions, dim3((unsigned)((n_a + 255) / 256)), dim3(256), 0, s, raw_a, (int)rows, ad, X, ldx,
                           a->act_off, (float)a->cfg.max_action);
        HP_CHECK_HIP(hipGetLastError());
        return (int)HP_OK;
    }, q_host);
}

int hp_agent_act(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, const double *obs_host, const double *g_host,
                 int64_t rows, double clip_obs, float *actions_host) {
    HP_REQUIRE(a && on && gn && obs_host && g_host && actions_host, HP_ERR_INVALID, "hp_agent_act: null argument");
    HP_SERIALISE(a);
    HP_TRY(check_policy_call("hp_agent_act", a, on, gn, net, true, rows));
    const double co = clip_or_inf(clip_obs);
    if (a->slab8) {
        HP_TRY(staged_policy_call(a, a->fwd_ws, a->ctx->stream, slab_net(a, net != HP_NET_ACTOR), norm_view(on), norm_view(gn), co,
                                  rows, obs_host, g_host, false, actions_host));
        HP_CHECK_HIP(hipStreamSynchronize(a->ctx->stream));
        return HP_OK;
    }
    const size_t nb_o = (size_t)rows * on->size * 8, nb_g = (size_t)rows * gn->size * 8;
    return actor_rows(a, net, rows, nb_o + nb_g, actions_host, [&](char *head, float *X, hipStream_t s) -> int {
        double *d_obs = reinterpret_cast<double *>(head), *d_g = reinterpret_cast<double *>(head + nb_o);
        HP_CHECK_HIP(hipMemcpyAsync(d_obs, obs_host, nb_o, hipMemcpyHostToDevice, s));
        HP_CHECK_HIP(hipMemcpyAsync(d_g, g_host, nb_g, hipMemcpyHostToDevice, s));
        return fill_policy_inputs(a, on, gn, d_obs, d_g, rows, co, X, s);
    });
}

int hp_agent_policy_snapshot(hp_agent *a, hp_norm *on, hp_norm *gn) {
    HP_REQUIRE(a && on && gn, HP_ERR_INVALID, "hp_agent_policy_snapshot: null argument");
    HP_SERIALISE(a);
    HP_REQUIRE(a->slab8, HP_ERR_STATE, "hp_agent_policy_snapshot: needs the fused policy kernel (slab8 engine)");
    HP_REQUIRE(on->size + gn->size == a->xdim, HP_ERR_INVALID, "hp_agent_policy_snapshot: normalizer sizes do not match the actor");
    hipStream_t s = a->ctx->stream;
    if (!a->act_stream) {
        HP_CHECK_HIP(hipStreamCreateWithFlags(&a->act_stream, hipStreamNonBlocking));
        HP_CHECK_HIP(hipEventCreateWithFlags(&a->act_done, hipEventDisableTiming));
        for (auto &ps : a->snap) {
            HP_CHECK_HIP(hipMalloc((void **)&ps.params, sizeof(float) * a->la.total));
            HP_CHECK_HIP(hipMalloc((void **)&ps.fragF, sizeof(float) * a->la.total));
            HP_CHECK_HIP(hipMalloc((void **)&ps.on, sizeof(NormDev)));
            HP_CHECK_HIP(hipMalloc((void **)&ps.gn, sizeof(NormDev)));
            HP_CHECK_HIP(hipEventCreateWithFlags(&ps.ready, hipEventDisableTiming));
        }
    }
    const int target = (a->snap_cur == 0) ? 1 : 0;        // never the set policy calls are reading
    hp_agent::PolicySnap &ps = a->snap[target];
    if (a->act_recorded) HP_CHECK_HIP(hipStreamWaitEvent(s, a->act_done, 0));
    const size_t nb = sizeof(float) * a->la.total;
    HP_CHECK_HIP(hipMemcpyAsync(ps.params, a->params, nb, hipMemcpyDeviceToDevice, s));
    HP_CHECK_HIP(hipMemcpyAsync(ps.fragF, a->fragF, nb, hipMemcpyDeviceToDevice, s));
    HP_CHECK_HIP(hipMemcpyAsync(ps.on, on->d, sizeof(NormDev), hipMemcpyDeviceToDevice, s));
    HP_CHECK_HIP(hipMemcpyAsync(ps.gn, gn->d, sizeof(NormDev), hipMemcpyDeviceToDevice, s));
    ps.clip_o = on->clip; ps.clip_g = gn->clip; ps.od = on->size; ps.gd = gn->size;
    HP_CHECK_HIP(hipEventRecord(ps.ready, s));
    a->snap_pending = target;
    return HP_OK;
}

int hp_agent_act_snapshot(hp_agent *a, const double *obs_host, const double *g_host, int64_t rows, double clip_obs,
                          float *actions_host) {
    HP_REQUIRE(a && obs_host && g_host && actions_host, HP_ERR_INVALID, "hp_agent_act_snapshot: null argument");
    HP_REQUIRE(rows > 0 && rows < (1 << 24), HP_ERR_INVALID, "hp_agent_act_snapshot: rows out of range");
    hipStream_t s = nullptr;
    {
        HP_SERIALISE(a);
        HP_REQUIRE(a->snap_cur >= 0 || a->snap_pending >= 0, HP_ERR_STATE, "hp_agent_act_snapshot: no snapshot taken yet");
        if (a->snap_pending >= 0) {
            hipEvent_t ev = a->snap[a->snap_pending].ready;
            hipError_t q = hipEventQuery(ev);
            if (q == hipErrorNotReady && a->snap_cur < 0) {   // the very first snapshot: nothing older to fall back to
                HP_CHECK_HIP(hipEventSynchronize(ev));
                q = hipSuccess;
            }
            (void)hipGetLastError();
            if (q == hipSuccess) {
                a->snap_cur = a->snap_pending;
                a->snap_pending = -1;
            }
        }
        const hp_agent::PolicySnap &ps = a->snap[a->snap_cur];
        s = a->act_stream;
        HP_TRY(staged_policy_call(a, a->act_ws, s, SlabNetPtrs{ps.fragF, nullptr, ps.params}, NormView{ps.on, ps.clip_o, ps.od},
                                  NormView{ps.gn, ps.clip_g, ps.gd}, clip_or_inf(clip_obs), rows, obs_host, g_host, false,
                                  actions_host));
        HP_CHECK_HIP(hipEventRecord(a->act_done, s));
        a->act_recorded = true;
    }
    HP_CHECK_HIP(hipStreamSynchronize(s));   // outside the context lock: the trainer keeps enqueueing meanwhile
    return HP_OK;
}

}  // extern "C"
