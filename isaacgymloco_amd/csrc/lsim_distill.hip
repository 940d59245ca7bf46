// lsim_distill.hip -- the loss joint of vision distillation (include/lsim.h, lsim_distill_loss) in liblsim.so.
// Compiled with the learner's flags (lsim_learn.hip: IEEE-rounded, denormals kept -- g = d * scale of a tiny d is numpy's value, which the
// tests compare bit for bit), but as a translation unit of its own: the learner's code object stays byte for byte what it was before this
// entry existed, so a caller that never distils runs exactly the kernels it ran (build.py).
#include <hip/hip_runtime.h>

#include "../../include/lsim.h"
#include "ls_distill.h"
