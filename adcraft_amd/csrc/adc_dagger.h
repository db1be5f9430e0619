// adc_dagger.h - the law of DAgger on the device (Ross, Gordon and Bagnell 2011, "A reduction of imitation learning and structured
// prediction to no-regret online learning"): days on which the learner, or a beta-mixture of learner and teacher, drives the env
// while the record keeps the teacher's action as the label.  Shared by the device kernel k_dagger_mix
// (parts/kernel_imitation.inc) and the host twin adc_dagger_coin_host (adc_shims.cpp); tests/dagger_ref.py restates these comments
// in numpy, bit for bit.
//
//   coin       env e on a DAgger day: w = draw(agent key of e, 0, ST_DAGGER = 23, 0, tick), tick the agent's tick BEFORE that
//              day's act (the act moves the tick on by one: a kernel behind the act reads tick - 1).  The teacher's action is
//              consumed iff bernoulli(w.x, bernoulli_threshold(beta)) - adc_law.h's, threshold = round(beta * 2^32) in
//              [0, 2^32]: beta = 1 always picks the teacher, beta = 0 never does.
//   state      none.  Key and tick are the ones the act's normals use (adc_mlp.h, stage ST_MLP): the coin follows the global env
//              id as the agent key does and resumes wherever the acts resume.  Stage 23 is drawn from by nothing else, so no env,
//              agent, TD3, SAC, ES, PBT, shuffle or PER stream moves.
//   label      the record's action of the day is the teacher's {budget, bids} whoever's action the step consumes (under the
//              bounded act in units of the box, mlp_unbox), logp = +0.
//   played     the step consumes the teacher's env-ready action where the coin picks the teacher and the learner's elsewhere.
#pragma once
#include "adc_mlp.h"

namespace adc {

constexpr uint32_t ST_DAGGER = 23;

// 1: the teacher's action is consumed.  threshold = bernoulli_threshold(beta), formed once per launch
ADC_HD bool dagger_coin(uint64_t key, uint32_t tick, uint64_t threshold)
{
    const U4 w = draw(key, 0u, ST_DAGGER, 0u, tick);
    return bernoulli(w.x, threshold);
}

}  // namespace adc
