// uavx_multi_launch.hpp -- from a handle to a launch: which kernel instantiation a handle runs (dispatch and the *Launch
// structs, ONE launch site per kernel family), the shape of its grids and workgroups.  Included by uavx_multi.hip at file scope
// (its contents sit in an anonymous namespace), behind uavx_multi_handle.hpp.

namespace {

// Kernel variant of a handle: compile-time agent count NT (1, 2, 4, 5, 8; 0 = runtime N), EXT (scripted bodies / curriculum),
// W wavefronts per workgroup (runtime-N path only).  dispatch() calls l.run<NT, EXT, W>() for the handle's variant.
template <class L>
int dispatch(const uavx_handle *h, const L &l) {
    if (h->ext) {   // bodies pin W = 1 (uavx_create); a curriculum alone keeps the mapping the agent count selected
        switch (h->gw) {
            case 2: return l.template run<0, true, 2>();
            case 3: return l.template run<0, true, 3>();
            case 4: return l.template run<0, true, 4>();
            default: return l.template run<0, true, 1>();
        }
    }
    switch (h->p.N) {
        case 1: return l.template run<1, false, 1>();
        case 2: return l.template run<2, false, 1>();
        case 4: return l.template run<4, false, 1>();
        case 5: return l.template run<5, false, 1>();   // (run_multi.py:5, test_pytorch_multi.py:27)
        case 8: return l.template run<8, false, 1>();
        default: break;
    }
    switch (h->gw) {
        case 2: return l.template run<0, false, 2>();
        case 3: return l.template run<0, false, 3>();
        case 4: return l.template run<0, false, 4>();
        default: return l.template run<0, false, 1>();
    }
}

// Tiles per workgroup of THIS launch: the handle's choice (uavx_create) as long as it runs the plain 8-UAV kernels.
inline int launch_tiles(const uavx_handle *h) { return (h->tiles == 2 && !h->ext && h->p.N == 8 && h->gw == 1) ? 2 : 1; }

// The switches known only at run time -- float64 commands, the polar-reference family, pairs of tiles, K > 1 -- choose between
// the addresses of a family's instantiations (they share one signature); the argument list of a family is written once.
// TMAX: 2 where the variant has a two-tile form (the plain 8-UAV kernels), else 1 -- both halves of pick() then name the same
// kernels.
template <class K>
K pick(bool pairs, bool f64, K pair64, K pair32, K one64, K one32) { return pairs ? (f64 ? pair64 : pair32) : (f64 ? one64 : one32); }

struct StepLaunch {
    uavx_handle *h; dim3 grid; hipStream_t st;
    const void *actions; int action_dtype, evaluate, K, tape_out;
    float *obs, *rew; uint8_t *done;
    template <int NT, bool EXT, int W> int run() const {
        constexpr int TMAX = (NT == 8 && !EXT && W == 1) ? 2 : 1;
        const bool f64 = action_dtype == UAVX_F64;
        const MultiParams &q = h->p;
        if (K == 1) {
            const int T = TMAX == 2 ? launch_tiles(h) : 1;   // pairs of one-wavefront tiles (uavx_create)
            const auto kernel = pick(T == 2, f64, &step_kernel<NT, true, EXT, W, TMAX>, &step_kernel<NT, false, EXT, W, TMAX>,
                                     &step_kernel<NT, true, EXT, W>, &step_kernel<NT, false, EXT, W>);
            return launch(h, kernel, dim3(grid.x / T), dim3(kWave * W * T), st, actions, static_cast<char *>(h->slab), h->off_vel, h->off_goal,
                          h->off_rec, h->off_wsteps, (uint32_t)q.E, (uint32_t)q.N, (uint32_t)q.epw, (uint32_t)q.magic, (uint32_t)q.nslots, q,
                          evaluate, obs, rew, done);
        }
        if constexpr (!EXT) {
            const auto kernel = f64 ? &step_k_kernel<NT, true, W> : &step_k_kernel<NT, false, W>;
            return launch(h, kernel, grid, dim3(kWave * W), st, q, actions, evaluate, K, tape_out, obs, rew, done);
        }
        return launched(h);   // (uavx_step_k refuses K > 1 with bodies / levels)
    }
};

struct StepExLaunch {
    uavx_handle *h; dim3 grid; hipStream_t st; StepExtra x; const uavx_step_args *a;
    // step_ex_ref_kernel (polar reference) or step_ex_kernel (cartesian / polar)
    template <int NT, bool EXT, int W> int run() const {
        constexpr int TMAX = (NT == 8 && !EXT && W == 1) ? 2 : 1;
        const int T = TMAX == 2 ? launch_tiles(h) : 1;   // (grid / stage_first / step_first were laid out in 128-thread workgroups by uavx_step_ex)
        const bool f64 = a->action_dtype == UAVX_F64;
        const auto kernel = a->action_mode == UAVX_ACTION_POLAR_REFERENCE
            ? pick(T == 2, f64, &step_ex_ref_kernel<NT, true, EXT, W, TMAX>, &step_ex_ref_kernel<NT, false, EXT, W, TMAX>,
                   &step_ex_ref_kernel<NT, true, EXT, W, 1>, &step_ex_ref_kernel<NT, false, EXT, W, 1>)
            : pick(T == 2, f64, &step_ex_kernel<NT, true, EXT, W, TMAX>, &step_ex_kernel<NT, false, EXT, W, TMAX>,
                   &step_ex_kernel<NT, true, EXT, W, 1>, &step_ex_kernel<NT, false, EXT, W, 1>);
        const uint32_t shape = (uint32_t)h->p.N | ((uint32_t)h->p.epw << 8) | ((uint32_t)h->p.nslots << 16);   // each <= 192
        return launch(h, kernel, grid, dim3(kWave * W * T), st, a->actions, static_cast<char *>(h->slab), h->off_vel, h->off_goal, h->off_rec,
                      h->off_wsteps, (uint32_t)h->p.E, x.stage_first, x.pf_blocks, x.step_first, shape, (uint32_t)h->p.magic, h->p, x,
                      a->evaluate, a->obs, a->rew, a->done);
    }
};

struct ObserveLaunch {
    uavx_handle *h; dim3 grid; hipStream_t st; float *obs;
    template <int NT, bool EXT, int W> int run() const {
        return launch(h, observe_kernel<NT, EXT, W>, grid, dim3(kWave * W), st, h->p, obs);
    }
};

struct ResetLaunch {
    uavx_handle *h; dim3 grid; hipStream_t st; const uint8_t *mask; uint64_t seed;
    template <int NT, bool EXT, int W> int run() const {
        return launch(h, reset_kernel<NT, EXT, W>, grid, dim3(kWave * W), st, h->p, mask, seed);
    }
};

// Wavefronts per workgroup for the runtime-N path.
// Measured (one box, bare step at 1.57 M agent slots, W = 1 / 2 / 3 / 4, profiles/r04_ab_notes.md section 12): a workgroup
// whose envs fill 64 W lanes EXACTLY (N = 3, 6, 12, 24, 48 with W = 3: every array of the workgroup's block starts and ends
// on a 64-byte sector and the obs / velocity tiles leave as whole 16-byte rows) gains 9-19 %; nearly-full pairs gain 7-10 % at
// N = 9, 10, 15, 20 and 37 % at N = 40; three wavefronts also at N = 7 and 11 (+9-10 %).  Five- and seven-wavefront
// workgroups (exact for N = 5, 10 / 7, 14) LOSE 8-30 % (not through their barriers: removing two of the three changed nothing).  Agent counts outside the table: the smallest W in 1..4 with the fewest idle lanes, if that beats one wavefront
// by more than 10 % (wider workgroups cost 0-2 % at W = 2 / 3 and 7-13 % at W = 4 where one wavefront is already aligned).
int pick_group_waves(int N) {
    if (N == 1 || N == 2 || N == 4 || N == 5 || N == 8) return 1;   // compile-time specialisations: one wavefront
    switch (N) {
        case 3: case 6: case 7: case 11: case 12: case 24: case 48: return 3;
        case 9: case 10: case 15: case 20: case 40: return 2;
        case 13: case 14: case 16: case 28: case 32: case 64: return 1;
        default: break;
    }
    const double u1 = (double)((kWave / N) * N) / kWave;
    double best = u1;
    int w = 1;
    for (int c = 2; c <= 4; c++) {
        const double u = (double)((kWave * c / N) * N) / (kWave * c);
        if (u > best + 1e-9) { best = u; w = c; }
    }
    return best > 1.10 * u1 ? w : 1;
}

dim3 wave_grid(const uavx_handle *h) {
    return dim3((unsigned)((h->p.E + h->p.epw - 1) / h->p.epw));  // one workgroup per epw envs
}
inline int64_t agent_slots(const uavx_handle *h) { return h->p.E * h->p.N; }

}  // namespace
