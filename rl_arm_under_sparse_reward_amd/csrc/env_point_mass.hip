// env_point_mass.hip -- the table row of the point-mass environment (PointMassEnvDev, env_device.h), and with it this kind's
// instantiation of the kernels of rollout_episodes.h.  One unit per kind: each compiles the policy slab's body once.
#include "rollout_episodes.h"

const EnvKind env_kind_point_mass = env_kind_entry<PointMassEnvDev>(HP_ENV_POINT_MASS);
