// adc_engine.hip - MI355X (gfx950) vectorised BiddingSimulation step engine: kernels + C ABI.
//
// The path (reference file:line it replaces):
//   BiddingSimulation.step                      adcraft/gymnasium_kw_env.py:160-269
//     simulate_epoch_of_bidding_on_campaign     adcraft/bidding_simulation.py:170-234
//       uniform_get_auctions_per_timestep       adcraft/bidding_simulation.py:151-167
//       simulate_epoch_of_bidding               adcraft/bidding_simulation.py:44-120
//         ImplicitKeyword.auction -> nth_price_auction   adcraft/synthetic_kw_classes.py:623-646,
//                                                        adcraft/synthetic_kw_helpers.py:116-180
//         ExplicitKeyword.auction                adcraft/synthetic_kw_classes.py:493-538, src/lib.rs:54-105
//     update_keywords                           adcraft/gymnasium_kw_env.py:114-158
//
// One translation unit (so the device log table and all inlining stay local without -fgpu-rdc), in parts:
//   parts/common.inc              device view of the engine (SoA pointers), wave scan/sum helpers, log table, drift
//   parts/kernel_fast.inc         k_step_implicit_fast - the budget-free pass for dense keyword sets.  One workgroup per (env,
//        256-keyword tile): phase 1 one lane per keyword (coalesced SoA loads, pending drift, volume draw, the keyword's two
//        exact win intervals in word space and its law records in LDS); phase 2 work items of 16 / 8 / 4 whole Philox calls
//        dealt lane-major, one word per auction, an auction = two subtract-and-compare pairs (stage A), clicked wins
//        compacted through per-wave LDS rings for the price + conversion / revenue call on full wavefronts (stage B),
//        integer-cent totals by LDS atomics; phase 3 coalesced observation stores.  Ignores the budget; exact whenever
//        the day's spend stays below it.
//   parts/kernel_sparse.inc       k_step_implicit_sparse - the same pass for keyword sets with few auctions per keyword (the
//        host's volume hint): auctions classified against conservative win BRACKETS (float estimates with a guaranteed
//        slack; the ~2e-5 of words in between take the long way), work items located through a byte list in LDS,
//        parameters / env header / metric sums software-pipelined across the tiles of a workgroup.
//   parts/kernel_exact_rows.inc   k_step_exact_rows - one workgroup per env: envs whose fast-pass spend reached the
//        budget are re-run in the reference's order, a sub-timestep row of K cells at a time (parallel cell
//        statistics, budget walk by prefix scans, ring-compacted conversions); then the step tail.
//        Since round 3 it stops at the row after the one the budget bound in and parks the env for k_step_rest_of_day (same file):
//        the remaining rows' auctions in whole Philox calls, wins counted by exact word intervals, the few cells that may hold
//        an affordable click walked in order.
//   parts/kernel_click_walk.inc   k_step_click_walk - binding budgets, K <= 256: the fast pass lists its clicked wins for envs whose
//        budget bound the day before; this kernel sorts the list into the reference's order (counting sort over the 24 x K
//        cells in LDS) and walks it - paid in full while the running total fits, click by click in the reference's float
//        arithmetic after - instead of re-running the day row by row.  Hands anything unusual to k_step_exact_rows.
//   parts/kernel_exact_serial.inc step_tail + k_step_exact - one wavefront per env walking cells serially: TAPE
//        replay of the reference's recorded variates, the EXPLICIT / IMPLICIT_GENERAL hand-overs, IMPLICIT with K > 2048, and the
//        read-only replay that regenerates a step's per-click lists (adc_engine_outcomes_replay).
//   parts/kernel_explicit_fast.inc the other two keyword models, keyword-parallel: k_step_explicit_fast, k_step_general_fast (the
//        reference's default ImplicitKeyword: top bids drawn as order statistics), k_step_float_day, k_step_explicit_rows.
//   parts/kernels_misc.inc        drift, metric sums, ideal profit, keyword generation, reset, synthetic actions,
//        flat observations/actions, nth_price_auction.
//   parts/kernels_policy.inc      the callers of the step on the device: the zero-margin agent, the per-step ideal profit on
//        the curves' contender lists (k_curve_contenders, k_ideal_from_contenders), the oracle bidder, per-env AKNCP / NCP.
//   parts/kernel_explicit_curves.inc  the bid curves and ideal profit of EXPLICIT keywords (k_explicit_curves: the two middle
//        normals of a keyword's cost samples by a radix select; k_explicit_curve_points); the policy kernels read them too.
//   parts/kernel_interp_agent.inc the interpolation agent (NaiveInterpolationStrategy): its caches, update and act
//        (k_interp_step); the per-keyword act itself is adc_interp.h, shared with the host twin.
//   parts/kernel_mlp_policy.inc   the learned agent: a fully connected policy (and value) network per env, or per member of a population.
//   parts/kernel_mlp_gru.inc      the recurrent learned agent: that policy with one GRU cell in front of its output layer, the state per env (adc_gru.h).
//   parts/kernel_es.inc           policy populations and the evolution strategy: perturbation, returns, gradient estimate + Adam (adc_es.h).
//   parts/kernel_pg.inc           policy-gradient training: GAE, the networks' backward pass, the weight gradient, the step (adc_pg.h);
//        the k_pg_pop_* twins run the same bodies for all members of a learner population in one launch.
//   parts/kernel_pg_kl.inc        the PPO learners' KL penalty and value-loss clip: the snapshot of the collecting distribution, the
//        sample pass's instantiations under the add-on (adc_pg_kl.h).
//   parts/kernel_pg_shuffle.inc   the PPO learners' shuffled sample-level minibatches: an epoch's order and record rows by a counter-addressed
//        permutation, the gathered instantiations of the sample pass and the weight gradient (adc_pg_shuffle.h).
//   parts/kernel_pg_queued.inc    the PPO / A2C learners' queued update: the stop and the clip scale decided on the device (k_pg_decide), the
//        chain's kernels that read a member's control block and pass a stopped member by.
//   parts/kernel_imitation.inc    imitation learning: the teacher's action into a teacher day's record slot (k_teach_record), the sample pass
//        of the behaviour-cloning / MARWIL loss (k_im_sample: pg_sample_body's instantiation kIm; adc_imitation.h), the label,
//        played action and mask of a DAgger day (k_dagger_mix; adc_dagger.h).
//   parts/kernel_td3.inc          off-policy training: the replay ring, the TD3 target, the twin critics, the actor's gradient (adc_td3.h);
//        the store, the target, the actor's pass and Polyak are td3_*_body functions that the solo kernel and its population twin both call.
//   parts/kernel_sac.inc          soft actor-critic: the soft target, the critics' pass, the actor's step, the temperature (adc_sac.h);
//        sac_target_body under k_sac_target and its population twin.
//   parts/kernel_td3_pop.inc      TD3 learner populations: the k_td3_pop_* twins, the member one more grid dimension; wrappers round
//        kernel_td3.inc's bodies with the member's row of the device tables.
//   parts/kernel_sac_pop.inc      SAC learner populations: the k_sac_pop_* twins of kernel_sac.inc, the member one more grid dimension;
//        the target a wrapper round sac_target_body, the critic and the actor kernel restated.
//   parts/kernel_per.inc          prioritised replay: the radix-64 sum tree's sample, weights, leaf update and node rebuild (adc_per.h).
//   parts/kernel_pbt.inc          population-based training over a learner population: the fitness from the record, the batched copy, SAC's temperature cells (adc_pbt.h).
//   parts/kernel_norm.inc         the running normalisers, one set of kernels: the record's batch moments of the observations in one pass,
//        the merge, the new vectors (adc_norm.h; over raw rows for the TD3 learners, adc_td3_norm.h); the discounted returns' scan under
//        the learner's discount, their moments, the merge, the multiplier, the GAE kernels under a multiplier and a clip (adc_rew_norm.h);
//        the batched copy.  The batch kernels of kernel_td3 / kernel_td3_pop and of kernel_sac / kernel_sac_pop (adc_sac_norm.h) normalise as they gather.
//   parts/host_api.inc            the engine's core on the host: the engine object, the env groups and their streams, owned allocations and
//                                 the holder of a call's temporaries (DevTemps), the step's launch and fetch, create and destroy, the
//                                 entry guards, and the entry points of the step itself.
//   parts/env_api.inc             the entry points that set or read the envs: parameters, keyword generation, reset, limits, drift, RNG
//                                 and episode state, buffers, env groups, the stream, flat actions and observations, the profile.
//   parts/tape_api.inc            the entry points of the tape replay and of the per-click outcome lists.
//   parts/curves_api.inc          the entry points of the episode metrics, the ideal profit, the bid curves and the oracle bidder.
//   parts/agent_api.inc           the entry points of the zero-margin agent and of the interpolation agent.
//   parts/selftest_api.inc        the device self-tests that take a device id and no engine, and the debug readers.
//   parts/mlp_core.inc            what the host files of the learned agent and the trainers' files share: owned allocations, the
//                                 agent's view and launch, a day of the agent, the parameter stores and the flat order against them,
//                                 the shared entry checks, the layer upload - and the lifetime chain (who ends when what ends).
//   parts/mlp_api.inc             the entry points of the learned agent: the single policy, populations, learners, squash and bounds.
//   parts/gru_api.inc             the entry points of the recurrent policy: its init, the cell's upload, the state's get, set and forget.
//   parts/es_api.inc              the entry points of the evolution strategy over a policy population.
//   parts/rollout_api.inc         the entry points of the rollout record and of the day loop (adc_engine_run_days).
//   parts/pg_core.inc             what the three policy-gradient host files share: the members (a single learner is one member), the
//                                 entry checks, the sample pass's view, the walk over the gradient's terms, the statistics' sums and
//                                 means, the LDS refusal, the trainer's allocation, a member's state by its flat offset.
//   parts/pg_kl_api.inc           the entry points of the KL penalty / value-clip add-on and what pg_api.inc calls of it, over pg_core.inc.
//   parts/pg_shuffle_api.inc      the entry points of the shuffled minibatches / target-KL stop add-on, the update under it, over pg_core.inc.
//   parts/pg_api.inc              the entry points of policy-gradient training, one function under the learner and the learner population:
//                                 the advantages, a minibatch, the host-driven and the queued update, over pg_core.inc.
//   parts/imitation_api.inc       the entry points of teacher days, DAgger days and of imitation learning over the single-learner trainer, over pg_core.inc.
//   parts/offpolicy_core.inc      what the four off-policy front ends share on the host: the ring, the critic upload, the state
//                                 vectors, the allocation, an update's launch helpers, the populations' update driver.
//   parts/td3_api.inc             the entry points of off-policy (TD3) training, over offpolicy_core.inc.
//   parts/sac_api.inc             the entry points of soft actor-critic training, over offpolicy_core.inc.
//   parts/td3_pop_api.inc         the entry points of TD3 learner populations, over offpolicy_core.inc.
//   parts/sac_pop_api.inc         the entry points of SAC learner populations, over offpolicy_core.inc.
//   parts/pbt_api.inc             the entry points of the population-based training scheduler over a PG, TD3 or SAC population.
//   parts/per_api.inc             the entry points of prioritised replay over a TD3 or SAC trainer, and what the trainers' updates call of it.
//   parts/nstep_api.inc           the entry points of n-step returns over a TD3 or SAC trainer (the store's window and the targets' gn are the kernels').
//   parts/norm_api.inc            the entry points of the running normalisers - observations, rewards, and the TD3 and SAC learners' as two
//                                 families of one front end - over shared helpers.
// The host-only exports - the `adcraft.rust` scalar shims, the host twins and the configuration checks - are the second source,
// adc_shims.cpp, in parts of its own: shims/<subsystem>.inc, named after the parts/*_api.inc they twin.
//
// No CPU path exists in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
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

namespace adck {
#include "parts/common.inc"
#include "parts/kernel_fast.inc"
#include "parts/kernel_sparse.inc"
#include "parts/kernel_exact_rows.inc"
#include "parts/kernel_click_walk.inc"
#include "parts/kernel_exact_serial.inc"
#include "parts/kernel_explicit_fast.inc"
#include "parts/kernels_misc.inc"
#include "parts/kernels_policy.inc"
#include "parts/kernel_explicit_curves.inc"
#include "parts/kernel_interp_agent.inc"
#include "parts/kernel_mlp_policy.inc"
#include "parts/kernel_mlp_gru.inc"
#include "parts/kernel_es.inc"
#include "parts/kernel_pg.inc"
#include "parts/kernel_pg_kl.inc"
#include "parts/kernel_pg_shuffle.inc"
#include "parts/kernel_pg_queued.inc"
#include "parts/kernel_imitation.inc"
#include "parts/kernel_td3.inc"
#include "parts/kernel_sac.inc"
#include "parts/kernel_td3_pop.inc"
#include "parts/kernel_sac_pop.inc"
#include "parts/kernel_pbt.inc"
#include "parts/kernel_per.inc"
#include "parts/kernel_norm.inc"
}  // namespace adck
using namespace adck;

#include "parts/host_api.inc"
#include "parts/env_api.inc"
#include "parts/tape_api.inc"
#include "parts/curves_api.inc"
#include "parts/agent_api.inc"
#include "parts/selftest_api.inc"
#include "parts/mlp_core.inc"
#include "parts/mlp_api.inc"
#include "parts/gru_api.inc"
#include "parts/es_api.inc"
#include "parts/rollout_api.inc"
#include "parts/pg_core.inc"
#include "parts/pg_kl_api.inc"
#include "parts/pg_shuffle_api.inc"
#include "parts/pg_api.inc"
#include "parts/imitation_api.inc"
#include "parts/offpolicy_core.inc"
#include "parts/td3_api.inc"
#include "parts/sac_api.inc"
#include "parts/td3_pop_api.inc"
#include "parts/td3_bounded_api.inc"
#include "parts/sac_pop_api.inc"
#include "parts/pbt_api.inc"
#include "parts/per_api.inc"
#include "parts/nstep_api.inc"
#include "parts/norm_api.inc"
#include "parts/comm_api.inc"
