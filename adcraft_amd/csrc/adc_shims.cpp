// adc_shims.cpp - the library's host-only exports: plain C++ with no HIP in it, compiled by hipcc into the library next to
// adc_engine.hip and by g++ into a host library of its own (oracle/build.py build_shims_host), so that CPU tests run the very code
// the GPU runs.  Three kinds of function, none on the per-step hot path: the scalar shims that mirror the reference's pyo3 module
// `adcraft.rust` (src/lib.rs); the host twins adc_*_host - the law headers (adc_*.h) the kernels call, on the caller's arrays; the
// checks adc_*_config_check that the engine's init entry points and engine.py call, whose sentences the caller sees
// (tests/golden/config_check_messages.json pins every one).  One translation unit, in parts named after the parts/*_api.inc they twin,
// included below in dependency order: a helper is defined in the part of the subsystem that owns it, before its first use.
//
// The reference's samplers draw from an unseeded thread_rng (src/lib.rs:25,43,61,75,320), so their individual values are not
// reproducible even by the reference; the shims take (seed, counter) and draw from the engine's Philox stream with the same float32
// transforms the kernels use.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../include/adcraft_engine.h"
#include "adc_law.h"
#include "adc_fast_schedule.h"
#include "adc_interp.h"
#include "adc_mlp.h"
#include "adc_gru.h"
#include "adc_es.h"
#include "adc_pg.h"
#include "adc_pg_kl.h"
#include "adc_pg_shuffle.h"
#include "adc_imitation.h"
#include "adc_dagger.h"
#include "adc_td3.h"
#include "adc_sac.h"
#include "adc_pbt.h"
#include "adc_norm.h"
#include "adc_rew_norm.h"
#include "adc_td3_norm.h"
#include "adc_sac_norm.h"
#include "adc_per.h"

#define ADC_EXPORT extern "C" __attribute__((visibility("default")))

// how every configuration check ends: msg = the first failing clause's sentence, or null
static inline int config_verdict(const char *msg, const char **message)
{
    if (message) *message = msg;
    return msg ? ADC_EINVAL : ADC_OK;
}

#include "shims/rust_scalar.inc"   // sigmoid, clamp, threshold_sigmoid, sums, the (seed, counter) samplers
#include "shims/law.inc"           // word-space win intervals, brackets, win bounds, offsets, dead keywords; the log table, the thread helper
#include "shims/fast_pass.inc"     // the dense fast pass: folded draws, proven prices, money packs, plain tiles, the queue tag, the schedule, the queue's protocol
#include "shims/keywords.inc"      // the EXPLICIT keyword sample and its cached bid curve
#include "shims/interp.inc"        // the interpolation agent's act
#include "shims/mlp.inc"           // the MLP policy: config check, stacked row, the act and the recurrent act (GRU), squash, bounds, math sweeps
#include "shims/es.inc"            // the evolution strategy: config check, noise, update; the optimiser's step record
#include "shims/norm.inc"          // the running normalisers: the moments, the four front ends' config checks, the ring families' normalised target
#include "shims/pg.inc"            // PPO / A2C: config check, the population checks' frame, GAE, the gradient core, decide, step
#include "shims/pg_kl.inc"         // the KL penalty and the value-loss clip
#include "shims/pg_shuffle.inc"    // the shuffled minibatches' order, the target-KL stop
#include "shims/imitation.inc"     // behaviour cloning / MARWIL weights and gradient, the DAgger coin
#include "shims/replay.inc"        // prioritised replay's sum tree, sample, priorities; the n-step window and targets
#include "shims/offpolicy.inc"     // what TD3 and SAC share: their common config clauses, a network's gradient terms, the critics' gradient
#include "shims/td3.inc"           // TD3: config checks, target, critic and actor gradients (free and bounded), Polyak
#include "shims/sac.inc"           // SAC: config checks, log-probability, soft target, gradients, the temperature step
#include "shims/pbt.inc"           // population-based training: config check, fitness, plan, explore
