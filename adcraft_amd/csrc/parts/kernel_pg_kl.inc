// kernel_pg_kl.inc - the PPO learners' KL penalty and value-loss clip on the device (the law is adc_pg_kl.h): the snapshot of the
// collecting distribution over the whole record, and the instantiations of kernel_pg.inc's sample pass that add the penalty's
// share to the policy network's output deltas, cap the value error and leave the add-on's own pieces.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  k_pg_old_dist is k_mlp_policy's shape with the policy network alone: one workgroup of 256 lanes per recorded row
// t * N + env, the row and every layer's outputs in LDS, mlp_layer's eight lanes per neuron - the law and the code of the act, so
// its means and log-stds are the act's bits.  The weight gradient, the joins and the step are kernel_pg.inc's, untouched: the
// add-on changes what the sample pass leaves in the deltas, nothing after it.

// what is a member's own under the add-on, indexed by member on the device
struct PgKlMember {
    adc::PgKl kl;
};

// floats of LDS of the snapshot: input row | the policy network's layer outputs
__host__ __device__ inline size_t pg_old_lds_floats(const adc::PgShape &sh)
{
    size_t n = (size_t)sh.D;
    for (int l = 0; l < sh.layers[0]; ++l) n += (size_t)sh.n_out[0][l];
    return n;
}

// recorded row `row` under the policy layers `net`: mean_old[row][A], and ls_old[row][A] with two heads
__device__ __forceinline__ void pg_old_dist_body(const adc::PgShape &sh, const MlpNet &net, const float *__restrict__ obs, size_t row,
                                                 float *__restrict__ mean_old, float *__restrict__ ls_old)
{
    extern __shared__ __align__(16) float pg_old_lds[];
    const int tid = threadIdx.x, A = sh.A, D = sh.D;
    float *x = pg_old_lds, *q = x + D;
    for (int j = tid; j < D; j += kPgBlock) x[j] = obs[row * (size_t)D + j];
    __syncthreads();
    const float *in = x;
    for (int l = 0; l < sh.layers[0]; ++l) {
        const bool last = l + 1 == sh.layers[0];
        mlp_layer(net.W[l], net.b[l], adc::pg_n_in(sh, 0, l), sh.n_out[0][l], in, q, last ? -1 : sh.activation);
        in = q;
        q += sh.n_out[0][l];
    }
    const float *o = in;
    for (int a = tid; a < A; a += kPgBlock) {
        mean_old[row * (size_t)A + a] = o[a];
        if (sh.two_heads) ls_old[row * (size_t)A + a] = adc::mlp_clamp_log_std(o[A + a], sh.clamp, sh.ls_lo, sh.ls_hi);
    }
}

// rows: T * N.  The free head's clamped log_std vector is copied by the first workgroup
__global__ __launch_bounds__(kPgBlock) void k_pg_old_dist(adc::PgShape sh, MlpNet net, const float *__restrict__ log_std, const float *__restrict__ obs,
                                                          float *__restrict__ mean_old, float *__restrict__ ls_old)
{
    pg_old_dist_body(sh, net, obs, blockIdx.x, mean_old, ls_old);
    if (!sh.two_heads && blockIdx.x == 0)
        for (int a = threadIdx.x; a < sh.A; a += kPgBlock) ls_old[a] = adc::mlp_clamp_log_std(log_std[a], sh.clamp, sh.ls_lo, sh.ls_hi);
}
// ... of a learner population: the row's env's member's layers; the first M workgroups copy a member's clamped log_std each
// (T * N >= M rows: every member has an env)
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_old_dist(adc::PgShape sh, const MlpLearner *__restrict__ learners, int N, int envs_per_member, int M,
                                                              const float *__restrict__ obs, float *__restrict__ mean_old, float *__restrict__ ls_old)
{
    const size_t row = blockIdx.x;
    const int member = (int)(row % (size_t)N) / envs_per_member;
    pg_old_dist_body(sh, learners[member].net[0], obs, row, mean_old, ls_old);
    if (!sh.two_heads && blockIdx.x < (unsigned)M) {
        const float *log_std = learners[blockIdx.x].log_std;
        for (int a = threadIdx.x; a < sh.A; a += kPgBlock)
            ls_old[(size_t)blockIdx.x * (size_t)sh.A + a] = adc::mlp_clamp_log_std(log_std[a], sh.clamp, sh.ls_lo, sh.ls_hi);
    }
}

// k_pg_sample / k_pg_pop_sample under the add-on
__global__ __launch_bounds__(kPgBlock) void k_pg_kl_sample(PgView p, PgKlView k, adc::PgKl kl)
{
    pg_sample_body<true>(p, p.net, p.log_std, p.loss, p.n0, blockIdx.x, blockIdx.x, k, kl, 0);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_kl_sample(PgView p, PgKlView k, const MlpLearner *__restrict__ learners, const PgMember *__restrict__ mem,
                                                               const PgKlMember *__restrict__ klmem, int envs_per_member)
{
    const int member = blockIdx.y;
    pg_sample_body<true>(p, learners[member].net, learners[member].log_std, mem[member].loss, p.n0 + member * envs_per_member, blockIdx.x,
                         (size_t)member * gridDim.x + blockIdx.x, k, klmem[member].kl, (size_t)member * (size_t)p.sh.A);
}
