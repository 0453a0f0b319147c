// env_pick_place.hip -- the table row of the pick-and-place environment (PickPlaceEnvDev, env_device.h), and with it this kind's
// instantiation of the kernels of rollout_episodes.h.  One unit per kind: each compiles the policy slab's body once.
#include "rollout_episodes.h"

const EnvKind env_kind_pick_place = env_kind_entry<PickPlaceEnvDev>(HP_ENV_PICK_PLACE);
