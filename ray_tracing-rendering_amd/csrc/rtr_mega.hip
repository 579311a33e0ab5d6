/*
 * rtr_mega.hip -- megakernel instantiations of one integrator group (see rt_launch.h); compiled three
 * times with -DRTR_MEGA_GROUP=0/1/2 so the variants build in parallel.
 *
 * Each group dispatches over the explicit list of its instantiations at the end of this file, one Row per
 * (I, T, M[, S][, PAIR]); every row stands for its three ACC twins, a PAIR row also for its job-queue twin k_mega_queue:
 * 46 rows (22 + 16 + 8), so 138 k_mega and 3 k_mega_queue, 141 kernels.  tests/test_kernel_variants.py holds the same
 * table and renders each of the 141 against the oracle: a variant added or removed here goes into that table too.
 */
#include "rt_kernels.h"
#include "rt_launch.h"

#ifndef RTR_MEGA_GROUP
#error "compile with -DRTR_MEGA_GROUP=0|1|2"
#endif

namespace {

int mega_fail(std::string& err, int code, const std::string& m) {
    err = m;
    return code;
}

int mega_status(hipError_t e, std::string& err) {
    return e == hipSuccess ? RTR_OK : mega_fail(err, RTR_ERR_DEVICE, std::string("megakernel launch: ") + hipGetErrorString(e));
}

/* MegaLaunch::prepare: what can fail without touching the stream, once per render; the kernel's own static LDS (a few
 * words of the workgroup vote) counts against the same 160 KiB */
template <typename K>
int prepare(K kernel, MegaLaunch& L, std::string& err) {
    hipFuncAttributes fa{};
    hipError_t e = hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel));
    if (e == hipSuccess)
        if (int rc = kernel_lds(kernel, L.lds, fa.sharedSizeBytes, err)) return rc;
    if (e == hipSuccess && L.occupancy) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&L.per_cu, kernel, RTR_BLOCK, L.lds);
    return mega_status(e, err);
}

template <typename K>
int launch_one(K kernel, MegaLaunch& L, std::string& err) {
    if (L.prepare) return prepare(kernel, L, err);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(L.P.n_tiles * L.P.chunks)), dim3(RTR_BLOCK), L.lds, L.stream, L.dsc, L.P, L.stack_words);
    return mega_status(hipGetLastError(), err);
}

/* the job-queue twin of a pair-cast variant: a persistent grid (MegaLaunch::queue) */
template <typename K>
int launch_queue(K kernel, MegaLaunch& L, std::string& err) {
    if (L.prepare) return prepare(kernel, L, err);
    const long long cells = (long long)L.P.n_tiles * L.P.chunks; /* four blocks each */
    long long grid = (long long)(L.per_cu > 0 ? L.per_cu : 1) * (L.n_cus > 0 ? L.n_cus : 1);
    if (grid > cells) grid = cells;
    if (L.grid_cap > 0 && grid > L.grid_cap) grid = L.grid_cap;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(RTR_BLOCK), L.lds, L.stream, L.dsc, L.P, L.stack_words,
                       reinterpret_cast<uint32_t*>(L.P.done + cells), (int)(cells * 4));
    return mega_status(hipGetLastError(), err);
}

/* one line of a group's list: k_mega<I, T, M, S, ACC, PR> for ACC = 0, 1, 2 */
template <int I, int T, int M, bool S = false, bool PR = false>
struct Row {
    static bool is(const MegaVariant& v) { return v.integ == I && v.trav == T && v.ms == M && v.sorted == S && v.pair == PR; }
    static int launch(MegaLaunch& L, std::string& err) {
        if constexpr (PR)
            if (L.queue) return launch_queue(k_mega_queue<I, T, M>, L, err);
        /* (an accumulator pass: the same variant with ACC = 1, or 2 with moments, rt_kernels.h) */
        return L.accum == 2 ? launch_one(k_mega<I, T, M, S, 2, PR>, L, err)
               : L.accum    ? launch_one(k_mega<I, T, M, S, 1, PR>, L, err)
                            : launch_one(k_mega<I, T, M, S, 0, PR>, L, err);
    }
};
/* the row that is MegaLaunch::variant, or RTR_ERR_UNSUPPORTED: never another kernel in its place */
template <typename... Rows>
int launch_from(MegaLaunch& L, std::string& err) {
    int rc = RTR_OK;
    if (((Rows::is(L.variant) && (rc = Rows::launch(L, err), true)) || ...)) return rc;
    const MegaVariant& v = L.variant;
    return mega_fail(err, RTR_ERR_UNSUPPORTED,
                     "no megakernel instantiation for integrator " + std::to_string(v.integ) + ", traversal " + std::to_string(v.trav) +
                         ", material set " + std::to_string(v.ms) + (v.sorted ? ", sorted" : "") + (v.pair ? ", pair cast" : ""));
}

} // namespace

#if RTR_MEGA_GROUP == 0
/* MIS: every traversal; lean / QuadLights-only / full material sets; the flat kernels have a pair-cast twin and the
 * flat QuadLights-only one a sorted twin */
int rtr_mega_launch_mis(MegaLaunch& L, std::string& err) {
    constexpr int I = RTR_INTEGRATOR_MIS;
    return launch_from<
        Row<I, RT_TRAV_FLAT, RT_MS_LEAN>,
        Row<I, RT_TRAV_FLAT, RT_MS_LEAN, false, true>,
        Row<I, RT_TRAV_FLAT, RT_MS_QUADLIT>,
        Row<I, RT_TRAV_FLAT, RT_MS_QUADLIT, false, true>,
        Row<I, RT_TRAV_FLAT, RT_MS_QUADLIT, true>,
        Row<I, RT_TRAV_FLAT, RT_MS_FULL>,
        Row<I, RT_TRAV_FLAT, RT_MS_FULL, false, true>,
        Row<I, RT_TRAV_FLAT_GUARD, RT_MS_QUADLIT>,
        Row<I, RT_TRAV_FLAT_GUARD, RT_MS_FULL>,
        Row<I, RT_TRAV_FAST, RT_MS_LEAN>,
        Row<I, RT_TRAV_FAST, RT_MS_QUADLIT>,
        Row<I, RT_TRAV_FAST, RT_MS_FULL>,
        Row<I, RT_TRAV_TOP, RT_MS_LEAN>,
        Row<I, RT_TRAV_TOP, RT_MS_QUADLIT>,
        Row<I, RT_TRAV_TOP, RT_MS_FULL>,
        Row<I, RT_TRAV_PROGRAM_EXT, RT_MS_QUADLIT>,
        Row<I, RT_TRAV_PROGRAM_EXT, RT_MS_FULL>,
        Row<I, RT_TRAV_PROGRAM, RT_MS_QUADLIT>,
        Row<I, RT_TRAV_PROGRAM, RT_MS_FULL>,
        Row<I, RT_TRAV_MEDIA, RT_MS_FULL>,
        Row<I, RT_TRAV_EXACT, RT_MS_LEAN>,
        Row<I, RT_TRAV_EXACT, RT_MS_FULL>>(L, err);
}
#elif RTR_MEGA_GROUP == 1
/* RR: every traversal, lean / full (it has no light code).  Path (like PBR and NEE): the generic
 * material set, one program kernel -- the general one --, and the media kernel, which also serves the reference-order
 * traversal of scenes without media */
int rtr_mega_launch_rr_path(MegaLaunch& L, std::string& err) {
    constexpr int R = RTR_INTEGRATOR_RR, P = RTR_INTEGRATOR_PATH;
    return launch_from<
        Row<R, RT_TRAV_FLAT, RT_MS_LEAN>,
        Row<R, RT_TRAV_FLAT, RT_MS_FULL>,
        Row<R, RT_TRAV_FLAT_GUARD, RT_MS_FULL>,
        Row<R, RT_TRAV_FAST, RT_MS_LEAN>,
        Row<R, RT_TRAV_FAST, RT_MS_FULL>,
        Row<R, RT_TRAV_TOP, RT_MS_LEAN>,
        Row<R, RT_TRAV_TOP, RT_MS_FULL>,
        Row<R, RT_TRAV_PROGRAM_EXT, RT_MS_FULL>,
        Row<R, RT_TRAV_PROGRAM, RT_MS_FULL>,
        Row<R, RT_TRAV_MEDIA, RT_MS_FULL>,
        Row<R, RT_TRAV_EXACT, RT_MS_LEAN>,
        Row<R, RT_TRAV_EXACT, RT_MS_FULL>,
        Row<P, RT_TRAV_FAST, RT_MS_FULL>,
        Row<P, RT_TRAV_TOP, RT_MS_FULL>,
        Row<P, RT_TRAV_PROGRAM_EXT, RT_MS_FULL>,
        Row<P, RT_TRAV_MEDIA, RT_MS_FULL>>(L, err);
}
#else
int rtr_mega_launch_pbr_nee(MegaLaunch& L, std::string& err) {
    constexpr int B = RTR_INTEGRATOR_PBR, N = RTR_INTEGRATOR_NEE;
    return launch_from<
        Row<B, RT_TRAV_FAST, RT_MS_FULL>,
        Row<B, RT_TRAV_TOP, RT_MS_FULL>,
        Row<B, RT_TRAV_PROGRAM_EXT, RT_MS_FULL>,
        Row<B, RT_TRAV_MEDIA, RT_MS_FULL>,
        Row<N, RT_TRAV_FAST, RT_MS_FULL>,
        Row<N, RT_TRAV_TOP, RT_MS_FULL>,
        Row<N, RT_TRAV_PROGRAM_EXT, RT_MS_FULL>,
        Row<N, RT_TRAV_MEDIA, RT_MS_FULL>>(L, err);
}
#endif
