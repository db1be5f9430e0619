// kernel_pg_queued.inc - a whole PPO / A2C update enqueued as one chain (adc_engine_pg_update_queued / _pg_pop_update_queued): the
// two decisions the host-driven update takes on the host between a minibatch's sums and its optimiser step - the target-KL stop and
// the norm clip's scale (adc_pg_shuffle.h: pg_decide) - taken on the device by k_pg_decide, and the instantiations of
// kernel_pg.inc's / kernel_pg_kl.inc's / kernel_pg_shuffle.inc's kernels that read what it decided from the device instead of their
// arguments.  The bodies are the shared ones (pg_sample_body, pg_wgrad_body, ...): a queued kernel is its host-driven twin with one
// read of the member's control block in front, uniform per workgroup, so a member that steps gets its twin's bits.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  k_pg_decide sits on the serial chain of every step between the sums' join and the optimiser step: one wave per member
// (a workgroup of 64 lanes, blockIdx.x = member), lane c < the number of sums copies sum c into the log, lane 0 alone runs the
// law - three float64 operations and two comparisons - and stores the control block.  A 256-lane block would add three idle waves
// to a kernel whose whole cost is its launch and one round trip to L2.  No atomics, no LDS; all stores are plain vector stores.
// Within the chain the stream's order is the only synchronisation: a control block is written by k_pg_decide alone and read by the
// kernels launched after it.

// a member's control block: what the chain's kernels read of the decisions taken so far in this update
struct PgQCtl {
    int stopped;                            // the member's update has stopped: every later kernel of the chain passes it by
    int taken;                              // optimiser steps decided in this update, the one about to run included
    int clip;                               // the step about to run: clip on / off, the clip scale
    float scale;
};
// a member's constants of the decision
struct PgQLaw {
    float max_grad_norm, target_kl;
};
// row (minibatch serial, member) of the log: the raw sums the host finishes after the one wait (adc_pg.h's ten, then the KL
// add-on's two while it lives), whether the member was live when the minibatch ran, and the minibatch's sample count
constexpr int kPgQSums = adc::kPgSums + adc::kPgKlPieces;
struct PgQRow {
    double sums[kPgQSums];
    int32_t evaluated, count;
};

// sums: [M][16] (pg_sums), nsums of a member's in use; row: the log's rows of this minibatch, one per member.  `taken` grows by at
// most one per launch: the host enqueues as many minibatches as a member's step table has rows, so taken - 1 stays within it
__global__ __launch_bounds__(kWave) void k_pg_decide(const double *__restrict__ sums, int nsums, int count, int stop_rule, const PgQLaw *__restrict__ law,
                                                     PgQCtl *__restrict__ ctl, PgQRow *__restrict__ row)
{
    const int member = blockIdx.x, lane = threadIdx.x;
    PgQCtl &c = ctl[member];
    PgQRow &r = row[member];
    if (c.stopped) {                        // (uniform per workgroup)
        if (lane == 0) r.evaluated = 0;
        return;
    }
    const double *mine = sums + (size_t)member * 16;
    if (lane < nsums) r.sums[lane] = mine[lane];
    if (lane != 0) return;
    r.evaluated = 1;
    r.count = count;
    const adc::PgDecision d = adc::pg_decide(law[member].max_grad_norm, law[member].target_kl, stop_rule, mine, (int64_t)count);
    if (d.stop) {
        c.stopped = 1;
        return;
    }
    c.clip = d.clip;
    c.scale = d.scale;
    c.taken = c.taken + 1;
}

// ---- the sample pass --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgBlock) void k_pg_q_sample(PgView p, const PgQCtl *__restrict__ ctl)
{
    if (ctl[0].stopped) return;
    pg_sample_body<false>(p, p.net, p.log_std, p.loss, p.n0, blockIdx.x, blockIdx.x, PgKlView{}, adc::PgKl{}, 0);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_q_kl_sample(PgView p, PgKlView k, adc::PgKl kl, const PgQCtl *__restrict__ ctl)
{
    if (ctl[0].stopped) return;
    pg_sample_body<true>(p, p.net, p.log_std, p.loss, p.n0, blockIdx.x, blockIdx.x, k, kl, 0);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_q_gather_sample(PgView p, const uint32_t *__restrict__ rows, const PgQCtl *__restrict__ ctl)
{
    if (ctl[0].stopped) return;
    pg_sample_body<false, true>(p, p.net, p.log_std, p.loss, 0, blockIdx.x, blockIdx.x, PgKlView{}, adc::PgKl{}, 0, rows);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_q_gather_kl_sample(PgView p, PgKlView k, adc::PgKl kl, const uint32_t *__restrict__ rows,
                                                                    const PgQCtl *__restrict__ ctl)
{
    if (ctl[0].stopped) return;
    pg_sample_body<true, true>(p, p.net, p.log_std, p.loss, 0, blockIdx.x, blockIdx.x, k, kl, 0, rows);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_q_sample(PgView p, const MlpLearner *__restrict__ learners, const PgMember *__restrict__ mem,
                                                              int envs_per_member, const PgQCtl *__restrict__ ctl)
{
    const int member = blockIdx.y;
    if (ctl[member].stopped) return;
    pg_sample_body<false>(p, learners[member].net, learners[member].log_std, mem[member].loss, p.n0 + member * envs_per_member, blockIdx.x,
                          (size_t)member * gridDim.x + blockIdx.x, PgKlView{}, adc::PgKl{}, 0);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_q_kl_sample(PgView p, PgKlView k, const MlpLearner *__restrict__ learners,
                                                                 const PgMember *__restrict__ mem, const PgKlMember *__restrict__ klmem,
                                                                 int envs_per_member, const PgQCtl *__restrict__ ctl)
{
    const int member = blockIdx.y;
    if (ctl[member].stopped) return;
    pg_sample_body<true>(p, learners[member].net, learners[member].log_std, mem[member].loss, p.n0 + member * envs_per_member, blockIdx.x,
                         (size_t)member * gridDim.x + blockIdx.x, k, klmem[member].kl, (size_t)member * (size_t)p.sh.A);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_q_gather_sample(PgView p, const MlpLearner *__restrict__ learners, const PgMember *__restrict__ mem,
                                                                     const uint32_t *__restrict__ rows, size_t rows_stride,
                                                                     const PgQCtl *__restrict__ ctl)
{
    const int member = blockIdx.y;
    if (ctl[member].stopped) return;
    pg_sample_body<false, true>(p, learners[member].net, learners[member].log_std, mem[member].loss, 0, blockIdx.x,
                                (size_t)member * gridDim.x + blockIdx.x, PgKlView{}, adc::PgKl{}, 0, rows + (size_t)member * rows_stride);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_q_gather_kl_sample(PgView p, PgKlView k, const MlpLearner *__restrict__ learners,
                                                                        const PgMember *__restrict__ mem, const PgKlMember *__restrict__ klmem,
                                                                        const uint32_t *__restrict__ rows, size_t rows_stride,
                                                                        const PgQCtl *__restrict__ ctl)
{
    const int member = blockIdx.y;
    if (ctl[member].stopped) return;
    pg_sample_body<true, true>(p, learners[member].net, learners[member].log_std, mem[member].loss, 0, blockIdx.x,
                               (size_t)member * gridDim.x + blockIdx.x, k, klmem[member].kl, (size_t)member * (size_t)p.sh.A,
                               rows + (size_t)member * rows_stride);
}

// ---- the weight gradient and its join ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgBlock) void k_pg_q_wgrad(PgTerm t, long long S, int B, int N, int n0, const float *__restrict__ deltas, int nd,
                                                         double *__restrict__ gpart, int Q, const PgQCtl *__restrict__ ctl)
{
    if (ctl[0].stopped) return;
    pg_wgrad_body(t, S, B, N, n0, deltas, nd, gpart, Q);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_q_gather_wgrad(PgTerm t, long long S, const uint32_t *__restrict__ rows, const float *__restrict__ deltas,
                                                                int nd, double *__restrict__ gpart, int Q, const PgQCtl *__restrict__ ctl)
{
    if (ctl[0].stopped) return;
    pg_wgrad_body<true>(t, S, 1, 0, 0, deltas, nd, gpart, Q, rows);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_q_wgrad(PgTerm t, long long S, int B, int N, int n0, int envs_per_member,
                                                             const float *__restrict__ deltas, int nd, double *__restrict__ gpart, int Q,
                                                             const PgQCtl *__restrict__ ctl)
{
    const size_t member = blockIdx.z, row0 = member * (size_t)S;
    if (ctl[member].stopped) return;
    if (!t.obs && t.X) t.X += row0 * t.ldx;
    pg_wgrad_body(t, S, B, N, n0 + (int)member * envs_per_member, deltas + row0 * (size_t)nd, nd, gpart + member * gridDim.y * (size_t)Q, Q);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_q_gather_wgrad(PgTerm t, long long S, const uint32_t *__restrict__ rows, size_t rows_stride,
                                                                    const float *__restrict__ deltas, int nd, double *__restrict__ gpart, int Q,
                                                                    const PgQCtl *__restrict__ ctl)
{
    const size_t member = blockIdx.z, row0 = member * (size_t)S;
    if (ctl[member].stopped) return;
    if (!t.obs && t.X) t.X += row0 * t.ldx;
    pg_wgrad_body<true>(t, S, 1, 0, 0, deltas + row0 * (size_t)nd, nd, gpart + member * gridDim.y * (size_t)Q, Q, rows + member * rows_stride);
}
// (one kernel for one learner and for a population: blockIdx.y = member, a single learner is member 0 of one)
__global__ __launch_bounds__(kPgBlock) void k_pg_q_grad_join(const double *__restrict__ gpart, int chunks, int Q, long long S, float *__restrict__ grad,
                                                             const PgQCtl *__restrict__ ctl)
{
    if (ctl[blockIdx.y].stopped) return;
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= Q) return;
    const double *mine = gpart + (size_t)blockIdx.y * (size_t)chunks * (size_t)Q;
    double total = 0.0;
    for (int c = 0; c < chunks; ++c) total = total + mine[(size_t)c * (size_t)Q + (size_t)p];
    grad[(size_t)blockIdx.y * (size_t)Q + (size_t)p] = adc::pg_grad_finish(total, S);
}

// ---- the statistics' sums: k_pg_pop_chunk_sums / k_pg_pop_join of a minibatch (inner = 0: the member's terms are its rows in order,
// modes 0 and 2), blockIdx.y / blockIdx.x = member ---------------------------------------------------------------------------------
__global__ void k_pg_q_chunk_sums(const float *__restrict__ src, int n, size_t mstep, int stride, int cols, int mode, double *__restrict__ part,
                                  size_t part_stride, const PgQCtl *__restrict__ ctl)
{
    const int lane = blockIdx.x * blockDim.x + threadIdx.x, member = blockIdx.y;
    if (ctl[member].stopped) return;
    const int chunks = (n + adc::kPgChunk - 1) / adc::kPgChunk;
    if (lane >= chunks * cols) return;
    const int chunk = lane / cols, col = lane % cols;
    const int i0 = chunk * adc::kPgChunk, i1 = i0 + adc::kPgChunk < n ? i0 + adc::kPgChunk : n;
    const size_t base = (size_t)member * mstep;
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) {
        const float x = src[(base + (size_t)i) * (size_t)stride + (size_t)col];
        acc = mode == 0 ? acc + (double)x : adc::pg_chain_mac(acc, x, x);
    }
    part[(size_t)member * part_stride + (size_t)lane] = acc;
}
__global__ void k_pg_q_join(const double *__restrict__ part, size_t part_stride, int chunks, int cols, double *__restrict__ out, int out_stride,
                            const PgQCtl *__restrict__ ctl)
{
    const int col = threadIdx.x, member = blockIdx.x;
    if (ctl[member].stopped) return;
    if (col >= cols) return;
    const double *mine = part + (size_t)member * part_stride;
    double total = 0.0;
    for (int c = 0; c < chunks; ++c) total = total + mine[(size_t)c * cols + col];
    out[(size_t)member * out_stride + col] = total;
}

// ---- the optimiser step: k_pg_update / k_pg_pop_update / k_pg_pop_update_live with the clip and its scale from the member's control
// block and the step's constants from row taken - 1 of the member's step table [steps_cap] (the host's pg_step_of for the steps
// s0 .. s0 + steps_cap - 1: c1 and c2 are the host's products, never recomputed here).  A stopped member's parameters, moments and
// control block stay as they are ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPgBlock) void k_pg_q_update(PgLayout L, float *__restrict__ theta, float *__restrict__ mom_m, float *__restrict__ mom_v,
                                                          const float *__restrict__ grad, const PgQCtl *__restrict__ ctl,
                                                          const adc::EsStep *__restrict__ steps)
{
    const PgQCtl c = ctl[0];
    if (c.stopped) return;
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    const adc::EsStep step = steps[c.taken - 1];
    float g = grad[p];
    if (c.clip) g = g * c.scale;
    float m = mom_m[p], v = mom_v[p];
    const float t1 = adc::pg_apply(step, theta[p], g, m, v);
    theta[p] = t1;
    mom_m[p] = m;
    mom_v[p] = v;
    *pg_param_slot(L, p) = t1;
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_q_update(PgLayout L, size_t stride, float *__restrict__ theta, float *__restrict__ mom_m,
                                                              float *__restrict__ mom_v, const float *__restrict__ grad,
                                                              const PgQCtl *__restrict__ ctl, const adc::EsStep *__restrict__ steps, int steps_cap)
{
    const size_t member = blockIdx.y;
    const PgQCtl c = ctl[member];
    if (c.stopped) return;
    const int p = blockIdx.x * kPgBlock + threadIdx.x;
    if (p >= L.Q) return;
    const adc::EsStep step = steps[member * (size_t)steps_cap + (size_t)(c.taken - 1)];
    const size_t i = member * (size_t)L.Q + (size_t)p;
    float g = grad[i];
    if (c.clip) g = g * c.scale;
    float m = mom_m[i], v = mom_v[i];
    const float t1 = adc::pg_apply(step, theta[i], g, m, v);
    theta[i] = t1;
    mom_m[i] = m;
    mom_v[i] = v;
    *(pg_param_slot(L, p) + member * stride) = t1;
}
