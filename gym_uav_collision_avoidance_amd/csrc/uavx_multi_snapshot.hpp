// uavx_multi_snapshot.hpp -- what is not the env API proper: the checkpoint format (uavx_snapshot_bytes / uavx_save / uavx_load)
// and uavx_selftest.  Included by uavx_multi.hip at file scope, last (snap_header_kernel is the last kernel of the translation
// unit).

extern "C" {

// ---- exact snapshot / restore of a handle (checkpoint row) ----
namespace {
constexpr uint64_t kSnapMagic = 0x3358564155ull;   // "UAVX3"
struct SnapHeader {
    uint64_t magic;
    uint32_t version, header_bytes;
    uint64_t slab_bytes, wide_bytes;
    int64_t E, env_offset;
    int32_t N, B, wide, ext, n_levels, level_lo, level_hi, prefetch_every;
    uint32_t world_version, epw;   // epw: envs per workgroup -- what the per-workgroup step counters of the slab are indexed by
    uavx_config cfg;
    uavx_body_rule rule;
    LevelTable levels;
};
size_t wide_slab_bytes(const uavx_handle *h) {   // the float64-position arrays (uavx_set_position_mode): 48 B per agent
    const size_t A = (size_t)h->p.E * h->p.N;
    return 2 * align_up(A * sizeof(double2), 256) + 2 * align_up(A * sizeof(double), 256);
}
size_t snap_header_bytes() { return align_up(sizeof(SnapHeader), 256); }
__global__ void snap_header_kernel(SnapHeader *dst, SnapHeader hd) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *dst = hd;
}
}  // namespace

int64_t uavx_snapshot_bytes(const uavx_handle *h) {
    if (!h) return -1;
    return (int64_t)(snap_header_bytes() + h->slab_bytes + wide_slab_bytes(h));
}

int uavx_save(uavx_handle *h, void *dst, void *stream) {
    if (!h || !dst) return UAVX_ERR_INVALID_ARG;
    if (reinterpret_cast<uintptr_t>(dst) & 255u) return fail(h, UAVX_ERR_INVALID_ARG, "uavx_save: the snapshot buffer must be 256-byte aligned");
    UAVX_ENTER(h);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SnapHeader hd;
    std::memset(&hd, 0, sizeof hd);
    hd.magic = kSnapMagic; hd.version = UAVX_VERSION; hd.header_bytes = (uint32_t)snap_header_bytes();
    hd.slab_bytes = h->slab_bytes; hd.wide_bytes = h->wide ? wide_slab_bytes(h) : 0;
    hd.E = h->p.E; hd.env_offset = h->p.env_offset; hd.N = h->p.N; hd.B = h->p.B; hd.wide = h->wide ? 1 : 0; hd.ext = h->ext ? 1 : 0;
    hd.n_levels = h->p.n_levels; hd.level_lo = h->p.level_lo; hd.level_hi = h->p.level_hi; hd.prefetch_every = h->prefetch_every;
    hd.world_version = h->p.world_version; hd.epw = (uint32_t)h->p.epw;
    hd.cfg = h->cfg; hd.rule = h->rule; hd.levels = h->levels;
    char *b = static_cast<char *>(dst);
    const int rc = launch(h, snap_header_kernel, dim3(1), dim3(64), st, reinterpret_cast<SnapHeader *>(b), hd);   // (by value: no host buffer to keep alive)
    if (rc != UAVX_OK) return rc;
    UAVX_HIP(h, hipMemcpyAsync(b + hd.header_bytes, h->slab, h->slab_bytes, hipMemcpyDeviceToDevice, st));
    if (h->wide) UAVX_HIP(h, hipMemcpyAsync(b + hd.header_bytes + h->slab_bytes, h->wide_slab, hd.wide_bytes, hipMemcpyDeviceToDevice, st));
    return UAVX_OK;
}

int uavx_load(uavx_handle *h, const void *src, void *stream) {
    if (!h || !src) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    hipStream_t st = static_cast<hipStream_t>(stream);
    SnapHeader hd;
    UAVX_HIP(h, hipMemcpyAsync(&hd, src, sizeof hd, hipMemcpyDeviceToHost, st));
    UAVX_HIP(h, hipStreamSynchronize(st));   // the header decides what follows: this call waits for `stream`
    if (hd.magic != kSnapMagic || hd.version != UAVX_VERSION || hd.header_bytes != snap_header_bytes())
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_load: not a snapshot of this library version");
    if (hd.E != h->p.E || hd.N != h->p.N || hd.B != h->p.B || hd.slab_bytes != h->slab_bytes || hd.epw != (uint32_t)h->p.epw)
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_load: the snapshot was taken from a handle of another shape (envs / agents / bodies / envs per workgroup)");
    // everything else the header carries goes into copy lengths, kernel arguments and table indices: a truncated or damaged
    // snapshot is refused here, not found out by a kernel
    const bool lvl_ok = hd.n_levels >= 0 && hd.n_levels <= UAVX_MAX_LEVELS &&
                        (hd.n_levels == 0 ? (hd.level_lo == -1 && hd.level_hi == -1)
                                          : (hd.level_lo < 0 || (hd.level_lo <= hd.level_hi && hd.level_hi < hd.n_levels)));
    if ((hd.wide != 0 && hd.wide != 1) || (hd.ext != 0 && hd.ext != 1) || hd.wide_bytes != (hd.wide ? wide_slab_bytes(h) : 0) ||
        !lvl_ok || hd.prefetch_every < 0 || hd.env_offset < 0 || !config_valid(&hd.cfg) || hd.cfg.num_agents != h->p.N ||
        hd.cfg.num_bodies != h->p.B || !(hd.rule.speed >= 0) || hd.rule.period < 1 || (hd.rule.period & (hd.rule.period - 1)) != 0 ||
        (hd.ext == 0 && (hd.B > 0 || hd.n_levels > 0)) || (hd.wide && hd.ext))
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_load: inconsistent snapshot header (truncated or corrupted snapshot)");
    const char *b = static_cast<const char *>(src);
    if (hd.wide) {   // the float64-position arrays exist from the first switch to that mode on
        const int rc = uavx_set_position_mode(h, UAVX_POS_F64, stream);
        if (rc != UAVX_OK) return rc;
    }
    UAVX_HIP(h, hipMemcpyAsync(h->slab, b + hd.header_bytes, h->slab_bytes, hipMemcpyDeviceToDevice, st));
    if (hd.wide) UAVX_HIP(h, hipMemcpyAsync(h->wide_slab, b + hd.header_bytes + h->slab_bytes, hd.wide_bytes, hipMemcpyDeviceToDevice, st));
    // host side of the handle: world, body rule, curriculum, staging cadence -- everything later launches take by value
    h->cfg = hd.cfg;
    derive_world_params(h->cfg, h->p);
    h->wl = derive_wide_limits(h->cfg);
    h->rule = hd.rule;
    apply_body_rule(h);
    h->levels = hd.levels;
    h->p.n_levels = hd.n_levels; h->p.level_lo = hd.level_lo; h->p.level_hi = hd.level_hi;
    h->p.world_version = hd.world_version;
    h->p.env_offset = hd.env_offset;      // the snapshot brings its own global env ids (the Philox streams are keyed by them)
    h->prefetch_every = hd.prefetch_every;
    h->ext = hd.ext != 0;
    h->wide = hd.wide != 0;
    return UAVX_OK;
}
int uavx_selftest(int device, uint64_t *mismatches) {
    if (!mismatches) return UAVX_ERR_INVALID_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return UAVX_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return UAVX_ERR_INVALID_ARG;
    DeviceGuard guard(device);
    if (guard.err != hipSuccess) return UAVX_ERR_HIP;
    unsigned long long *d = nullptr, h = 0;
    if (hipMalloc(&d, sizeof h) != hipSuccess) return UAVX_ERR_ALLOC;
    hipError_t e = hipMemset(d, 0, sizeof h);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sqrt_selftest_kernel, dim3(256 * 32), dim3(256), 0, 0, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return UAVX_ERR_HIP;
    *mismatches = h;
    return UAVX_OK;
}

}  // extern "C"
