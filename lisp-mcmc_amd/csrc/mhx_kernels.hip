// mhx_kernels.hip -- the ahead-of-time compiled gfx950 kernels, built once per kernel family: device
// code in mhx_kernels.hpp (shared with the run-time compiled user-expression kernels), the
// model-free read-out kernels in mhx_readout_kernels.hpp (the primary family's unit alone), spec
// table and launchers in mhx_launch.inc.
#include "mhx_kernels.hpp"
#ifdef MHX_FAMILY_PRIMARY
#include "mhx_readout_kernels.hpp"
#endif

#include "mhx_launch.inc"
