// env_push_block.hip -- the table row of the push-block environment (PushBlockEnvDev, env_device.h), and with it this kind's
// instantiation of the kernels of rollout_episodes.h.  One unit per kind: each compiles the policy slab's body once.
#include "rollout_episodes.h"

const EnvKind env_kind_push_block = env_kind_entry<PushBlockEnvDev>(HP_ENV_PUSH_BLOCK);
