#pragma once
// vbn_walk_impl.h -- gfx950 (MI355X) particle walk for batched Bayesian-network inference: the
// device code and the vbn_walk_kernel template, shared by vbn_walk.hip (host entry points),
// walk_inst.hip (one kind-set instantiation per object, built in parallel) and the
// plan-specialised units (vbn_walk_plan.h).  The parts, in the order they build on each other:
#include "vbn_walk_common.h"   // vbn_step accessors, RNG, Lane, slot / evidence reads, staging constants
#include "vbn_walk_mlp.h"      // the NN CPDs' MLP
#include "vbn_walk_cpd.h"      // gaussian_nn, linear_gaussian, mdn, softmax_nn steps
#include "vbn_walk_kde.h"      // the kde step and its moment tables
#include "vbn_walk_kernel.h"   // Gibbs roles, walk_step, staging, statistics epilogue, the kernel
