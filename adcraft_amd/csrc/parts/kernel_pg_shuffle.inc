// kernel_pg_shuffle.inc - the PPO / A2C learners' shuffled sample-level minibatches on the device (the law is adc_pg_shuffle.h): an
// epoch's order and record rows of every member in one launch, the gathered instantiations of kernel_pg.inc's sample pass (with
// and without the KL add-on) and weight gradient, and the population's step that leaves a stopped member as it is.
// (part of the single translation unit adc_engine.hip)
// -------------------------------------------------------------------------------------------------
// Shape.  k_pg_shuffle_rows: one lane per position of a member's order (blockIdx.y = member) walks the Feistel cycle - four Philox
// calls per application, under four applications expected - and writes the sample index and its record row with plain vector
// stores.  The walk's trip count differs per lane; at a few thousand to a few hundred thousand positions per epoch the kernel is
// a few microseconds of a whole epoch's minibatches and is left as it is.  The gathered sample pass and weight gradient are the
// bodies of kernel_pg.inc with the record row read from rows[member][j * mb + s] instead of computed from (s, B, N, n0): the same
// bytes of the record with less locality (a sample's observation row is still one contiguous read of D floats).

// what is a member's own under the add-on, indexed by member on the device: its key, and the tick its next order is drawn with
struct PgShuffleMember {
    uint64_t key;
    uint32_t tick, pad;
};

// order[member][i] = sigma(i), rows[member][i] = its record row; n_s = T * n positions per member
__global__ __launch_bounds__(256) void k_pg_shuffle_rows(const PgShuffleMember *__restrict__ mem, uint32_t n_s, uint32_t half_bits, uint32_t n, uint32_t N,
                                                         uint32_t *__restrict__ order, uint32_t *__restrict__ rows)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, member = blockIdx.y;
    if (i >= n_s) return;
    const PgShuffleMember c = mem[member];
    const uint32_t x = adc::pg_shuffle_sample(c.key, i, n_s, half_bits, c.tick);
    const size_t at = (size_t)member * (size_t)n_s + (size_t)i;
    order[at] = x;
    rows[at] = adc::pg_shuffle_row(x, n, N, member);
}

// the sample pass over gathered rows: sample blockIdx.x of the minibatch is record row rows[blockIdx.x] (p.B and p.n0 are not read)
__global__ __launch_bounds__(kPgBlock) void k_pg_gather_sample(PgView p, const uint32_t *__restrict__ rows)
{
    pg_sample_body<false, true>(p, p.net, p.log_std, p.loss, 0, blockIdx.x, blockIdx.x, PgKlView{}, adc::PgKl{}, 0, rows);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_gather_kl_sample(PgView p, PgKlView k, adc::PgKl kl, const uint32_t *__restrict__ rows)
{
    pg_sample_body<true, true>(p, p.net, p.log_std, p.loss, 0, blockIdx.x, blockIdx.x, k, kl, 0, rows);
}
// ... of member blockIdx.y: its rows start rows_stride further per member, its scratch rows at member * gridDim.x
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_gather_sample(PgView p, const MlpLearner *__restrict__ learners, const PgMember *__restrict__ mem,
                                                                   const uint32_t *__restrict__ rows, size_t rows_stride)
{
    const int member = blockIdx.y;
    pg_sample_body<false, true>(p, learners[member].net, learners[member].log_std, mem[member].loss, 0, blockIdx.x,
                                (size_t)member * gridDim.x + blockIdx.x, PgKlView{}, adc::PgKl{}, 0, rows + (size_t)member * rows_stride);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_gather_kl_sample(PgView p, PgKlView k, const MlpLearner *__restrict__ learners,
                                                                      const PgMember *__restrict__ mem, const PgKlMember *__restrict__ klmem,
                                                                      const uint32_t *__restrict__ rows, size_t rows_stride)
{
    const int member = blockIdx.y;
    pg_sample_body<true, true>(p, learners[member].net, learners[member].log_std, mem[member].loss, 0, blockIdx.x,
                               (size_t)member * gridDim.x + blockIdx.x, k, klmem[member].kl, (size_t)member * (size_t)p.sh.A,
                               rows + (size_t)member * rows_stride);
}

// the weight gradient over gathered rows: only the observation term reads the record; acts, deltas and partials stay indexed by slot
__global__ __launch_bounds__(kPgBlock) void k_pg_gather_wgrad(PgTerm t, long long S, const uint32_t *__restrict__ rows, const float *__restrict__ deltas,
                                                              int nd, double *__restrict__ gpart, int Q)
{
    pg_wgrad_body<true>(t, S, 1, 0, 0, deltas, nd, gpart, Q, rows);
}
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_gather_wgrad(PgTerm t, long long S, const uint32_t *__restrict__ rows, size_t rows_stride,
                                                                  const float *__restrict__ deltas, int nd, double *__restrict__ gpart, int Q)
{
    const size_t member = blockIdx.z, row0 = member * (size_t)S;
    if (!t.obs && t.X) t.X += row0 * t.ldx;
    pg_wgrad_body<true>(t, S, 1, 0, 0, deltas + row0 * (size_t)nd, nd, gpart + member * gridDim.y * (size_t)Q, Q, rows + member * rows_stride);
}

// k_pg_pop_update that leaves a member whose update has stopped (PgMember.stopped) bit for bit as it is
__global__ __launch_bounds__(kPgBlock) void k_pg_pop_update_live(PgLayout L, size_t stride, float *__restrict__ theta, float *__restrict__ mom_m,
                                                                 float *__restrict__ mom_v, const float *__restrict__ grad,
                                                                 const PgMember *__restrict__ mem)
{
    if (mem[blockIdx.y].stopped) return;
    pg_pop_update_body(L, stride, theta, mom_m, mom_v, grad, mem);
}
