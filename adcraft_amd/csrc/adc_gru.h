// adc_gru.h - the law of the recurrent MLP policy: the feed-forward policy of adc_mlp.h with one GRU cell of width G (1..256) in
// front of its output layer, and the per-env state that cell carries from one act to the next.  Shared by the device kernel
// (parts/kernel_mlp_gru.inc) and the host twins adc_gru_cell_host / adc_mlp_act_recurrent_host / adc_gru_state_host
// (adc_shims.cpp), so that CPU tests run the very operations the GPU runs; tests/gru_ref.py restates these comments in numpy, bit
// for bit.
//
// Every float32 value below is the result of ONE correctly rounded IEEE operation (build with -ffp-contract=off); "f64" marks
// the few places that compute in float64 and round once.  sum8, tanh (mlp_tanh), exp64 and the weight layout are adc_mlp.h's.
//
//   network    n_policy_layers = L.  Layers 0 .. L-2 are the trunk, as in adc_mlp.h, the activation after each.  The cell's input
//              x is the trunk's last activation, or the network's (normalised) input row when L = 1; n_in is its length.  The
//              output layer L-1 has n_in = G and reads the new state h'.  There is no activation after the cell.
//   cell       torch.nn.GRUCell's arithmetic, gates in the order r, z, n; gate row q = gate * G + g, g < G:
//                  gi[q] = sum8(n_in, j -> Wi[j][q] * x[j]) + bi[q]        q < 3G
//                  gh[q] = sum8(G,    j -> Wh[j][q] * h[j]) + bh[q]
//                  r  = sigmoid(gi[g]     + gh[g])
//                  z  = sigmoid(gi[G + g] + gh[G + g])
//                  t  = r * gh[2G + g];  n = tanh(gi[2G + g] + t)
//                  u  = 1 - z;  p = u * n;  s = z * h[g];  h'[g] = p + s
//              Wi [n_in][3G] and Wh [G][3G] are stored as two chain-major layers with n_out = 3G (mlp_weight_index).
//   sigmoid(v) float32 -> float32: a = min(max(v, -87), 88) as f64; result = float32(1 / (1 + exp64(-a))).  NaN -> NaN.
//   state      h[N][2][G] float32 and two words per env, last (the episode day of the last act; -2: none) and from, under the
//              observation history's rule (adc_mlp.h mlp_hist_from).  An act on episode day d:
//                  from = mlp_hist_from(d, last, from)      (d == 0: 0; last neither d - 1 nor d: d; else unchanged)
//                  the input state is zeros if from == d, else slot (d + 1) & 1
//                  h' goes to slot d & 1 (after a barrier: every read of the workgroup is behind it); last = d
//              from == d covers day 0, an auto-reset, a gap of days stepped without the agent and the first act after an explicit
//              reset (adc_engine_reset sets last = -2 for the envs it resets; adc_engine_mlp_hidden_forget and
//              adc_engine_es_perturb for every env).  A second act on the same day (replayed normals) reads the same input state -
//              the other slot, or zeros again - and writes the same bits.  One case is not detected, as in the history: an
//              auto-reset followed by exactly last + 1 days without an act reads the old episode's state as the new one's.
//   the rest   everything after the output layer is adc_mlp.h untouched: heads, sample, log-probability, bid, budget.  The value
//              network stays the feed-forward one on the input row.  No squash, no bounds, no observation history (frames = 1).
//   flat order (adc_es.h's, for the strategy): the trunk layers, Wi input-major (j * 3G + q) then bi, Wh then bh, the output layer.
#pragma once
#include "adc_mlp.h"

namespace adc {

constexpr int kGruMaxWidth = 256;
// floats of LDS beyond the feed-forward policy's: the state | gi | gh
ADC_HD size_t gru_lds_floats(int G) { return (size_t)7 * (size_t)G; }

ADC_HD float gru_sigmoid(float v)
{
    if (v != v) return v;
    v = v < -87.0f ? -87.0f : v;
    v = v > 88.0f ? 88.0f : v;
    const double e = mlp_exp64(-(double)v);
    return (float)(1.0 / (1.0 + e));
}

// unit g of the cell from its six pre-activations and its old state
ADC_HD float gru_unit(float gi_r, float gh_r, float gi_z, float gh_z, float gi_n, float gh_n, float h)
{
    const float r = gru_sigmoid(gi_r + gh_r);
    const float z = gru_sigmoid(gi_z + gh_z);
    const float t = r * gh_n;
    const float n = mlp_tanh(gi_n + t);
    const float u = 1.0f - z;
    const float p = u * n;
    const float s = z * h;
    return p + s;
}

// the state rule: an act on episode day d under `from` (mlp_hist_from of the env's words) starts from zeros, or reads a slot
ADC_HD bool gru_starts_from_zeros(int32_t d, int32_t from) { return from == d; }
ADC_HD int gru_read_slot(int32_t d) { return (int)((d + 1) & 1); }
ADC_HD int gru_write_slot(int32_t d) { return (int)(d & 1); }

}  // namespace adc
