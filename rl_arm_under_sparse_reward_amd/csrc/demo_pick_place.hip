// demo_pick_place.hip -- the pick-and-place environment's instantiation of the scripted-episode kernel (demo_episodes.h): the
// third launch of its table row (env_pick_place.hip).  A unit of its own: it needs no policy slab, and the unit of the rollout
// kernels compiles what it compiled before.
#include "demo_episodes.h"

template hipError_t env_launch_demo<PickPlaceEnvDev>(hipStream_t, unsigned, const DemoArgs &);
