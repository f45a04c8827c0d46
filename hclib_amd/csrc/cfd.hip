// cfd.hip — Rodinia CFD (test/performance-regression/full-apps/rodinia/cfd:
// euler3d_cpu_double.cpp the HClib port, euler3d_cpu_double.ref.cpp the
// arithmetic) as one launch of the generic device promise DAG
// (include/hclib_hip/hx_dag.h, run_dag_group).
//
// The reference runs 1 + 5 (2 + 3 * 2) = 41 hclib_forasync_future sweeps over
// all elements, each followed by hclib_future_wait (euler3d_cpu_double.cpp
// :74-79, 147-152, 228-233, 294-299, 460-465). Here a task is one block of
// elements in one Runge-Kutta stage, it awaits the blocks its elements'
// faces name and the blocks that name it, of the stage before, and nothing
// else (hx_cfd_plan.h has the graph and the argument that these awaits order
// the overwrites of the two state buffers and of old / step_factors):
//
//   task (s, b), j = s % 3              awaits                    puts
//   reads  buffer s & 1: b's elements   (s - 1, b') for b' in     (s, b)
//          and their neighbours;        N(b), the symmetrised
//          j > 0: old, step_factors     neighbourhood of b
//   writes buffer (s + 1) & 1, b's elements; j == 0: old, step_factors
//
// The body. One workgroup of four waves per task, threads striding over the
// block's elements, an element per thread at a time: the element's state, its
// four faces' neighbour states (all loads ahead of the arithmetic), the step
// factor (:186-200) where j == 0, the flux (:225-343) face by face in the
// reference's order, each face the neighbour branch, the wing branch or the
// far-field branch, and the time step (:356-362). `fluxes` stays in registers.
//
// Arithmetic: __dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn, every
// operation rounded on its own in the reference's operand order (an x86-64
// build of the reference without -march has no fused multiply-add).
//
// Memory protocol. The two state buffers, old and step_factors are written and
// read by different workgroups during the launch: every access is an
// agent-scope (sc1) load or write-through store, the payload form run_dag_group
// hands from task to task behind a drain and a barrier (kSc1Payload, as
// jacobi.hip). Areas, neighbour indices and normals are uploaded before the
// launch and only read: plain loads. Device layout of state and old: one array
// per variable, each on a 256-byte line (a wave's own loads and stores are
// whole lines; a neighbour gather touches five), or, HCLIB_HIP_CFD_LAYOUT=0,
// 8 doubles per element, 5 used (a gather is half a 128-byte line; stored as
// two 16-byte stores and one of 8). The array per variable measured faster in
// every configuration (DESIGN.md §22 has the record). Neighbours that lie in
// the task's own block are gathered from memory like the others, not from LDS:
// that variant was not built.
//
// The phases form runs the same element body as one plain kernel per stage,
// stream-ordered from the host: the reference's join-per-sweep schedule, for
// comparison. Same bits.
#include <string.h>

#include <vector>

#include "hx_cfd_host.h"
#include "hx_cfd_plan.h"
#include "hx_client.h"

namespace hx {
namespace {

constexpr int kCfdThreads = 256;

struct CfdCtx {
    const double *areas;
    const int *nbs;
    const double *normals;
    double *var[2];  // the ping-pong state buffers
    double *old, *sf;
    uint32_t *err;  // the launch's device error word (dag form)
    CfdFarField ff;
    size_t es, vs;  // index of variable k of element i: i es + k vs
    int nelr, block, stages;
};

__device__ __forceinline__ double fa(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double fs(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double fm(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double fdv(double a, double b) { return __ddiv_rn(a, b); }
__device__ __forceinline__ double fq(double a) { return __dsqrt_rn(a); }

// What compute_velocity, compute_speed_sqd, compute_pressure,
// compute_speed_of_sound and compute_flux_contribution (:136-176) make of a state
struct CfdDerived {
    double ssq, p, c;
    double fmom[3][3];  // flux_contribution_momentum_{x,y,z}.{x,y,z}
    double fe[3];       // flux_contribution_density_energy
};

__device__ __forceinline__ void cfd_derive(const double (&v)[5], CfdDerived &d) {
    const double vx = fdv(v[1], v[0]), vy = fdv(v[2], v[0]), vz = fdv(v[3], v[0]);
    d.ssq = fa(fa(fm(vx, vx), fm(vy, vy)), fm(vz, vz));
    d.p = fm(fs(double(1.4), double(1.0)), fs(v[4], fm(fm(double(0.5), v[0]), d.ssq)));
    d.c = fq(fdv(fm(double(1.4), d.p), v[0]));
    d.fmom[0][0] = fa(fm(vx, v[1]), d.p);
    d.fmom[0][1] = fm(vx, v[2]);
    d.fmom[0][2] = fm(vx, v[3]);
    d.fmom[1][0] = d.fmom[0][1];
    d.fmom[1][1] = fa(fm(vy, v[2]), d.p);
    d.fmom[1][2] = fm(vy, v[3]);
    d.fmom[2][0] = d.fmom[0][2];
    d.fmom[2][1] = d.fmom[1][2];
    d.fmom[2][2] = fa(fm(vz, v[3]), d.p);
    const double de_p = fa(v[4], d.p);
    d.fe[0] = fm(vx, de_p);
    d.fe[1] = fm(vy, de_p);
    d.fe[2] = fm(vz, de_p);
}

// "accumulate cell-centered fluxes" (:285-305, :315-334): the other side's
// momentum and flux contributions against the element's, normal component by
// component
__device__ __forceinline__ void cfd_accumulate(const double (&n)[3], const double *mom_o, const double (&fmom_o)[3][3],
                                               const double (&fe_o)[3], const double (&v)[5], const CfdDerived &d,
                                               double (&flux)[5]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double factor = fm(double(0.5), n[k]);
        flux[0] = fa(flux[0], fm(factor, fa(mom_o[k], v[1 + k])));
        flux[4] = fa(flux[4], fm(factor, fa(fe_o[k], d.fe[k])));
        flux[1] = fa(flux[1], fm(factor, fa(fmom_o[0][k], d.fmom[0][k])));
        flux[2] = fa(flux[2], fm(factor, fa(fmom_o[1][k], d.fmom[1][k])));
        flux[3] = fa(flux[3], fm(factor, fa(fmom_o[2][k], d.fmom[2][k])));
    }
}

// element i of stage s (j = s % 3)
__device__ __forceinline__ void cfd_element(const CfdCtx &c, int s, int j, int i) {
    const double *src = c.var[s & 1];
    double *dst = c.var[(s + 1) & 1];
    const size_t es = c.es, vs = c.vs, at = (size_t)i * es;

    // every load of the element ahead of its arithmetic
    const int4 nb4 = *(const int4 *)&c.nbs[(size_t)i * kCfdNnb];
    const int nb[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
    double v[5], o[5], w[4][5], nrm[4][3], step;
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] = ld_agent(&src[at + k * vs]);
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int k = 0; k < 5; ++k) w[f][k] = nb[f] >= 0 ? ld_agent(&src[(size_t)nb[f] * es + k * vs]) : 0.0;
    if (j != 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k) o[k] = ld_agent(&c.old[at + k * vs]);
        step = ld_agent(&c.sf[i]);
    }
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int k = 0; k < 3; ++k) nrm[f][k] = c.normals[((size_t)i * kCfdNnb + f) * kCfdNdim + k];

    CfdDerived d;
    cfd_derive(v, d);
    if (j == 0) {
        // copy and compute_step_factor (:186-200)
        step = fdv(double(0.5), fm(fq(c.areas[i]), fa(fq(d.ssq), d.c)));
#pragma unroll
        for (int k = 0; k < 5; ++k) o[k] = v[k];
        st_agent(&c.sf[i], step);
        if (vs == 1) {
            st_sc1_x4(&c.old[at], make_uint4((uint32_t)__double2loint(o[0]), (uint32_t)__double2hiint(o[0]),
                                             (uint32_t)__double2loint(o[1]), (uint32_t)__double2hiint(o[1])));
            st_sc1_x4(&c.old[at + 2], make_uint4((uint32_t)__double2loint(o[2]), (uint32_t)__double2hiint(o[2]),
                                                 (uint32_t)__double2loint(o[3]), (uint32_t)__double2hiint(o[3])));
            st_agent(&c.old[at + 4], o[4]);
        } else {
#pragma unroll
            for (int k = 0; k < 5; ++k) st_agent(&c.old[at + k * vs], o[k]);
        }
    }

    // compute_flux (:225-343)
    const double smoothing_coefficient = double(0.2f);
    const double speed_i = fq(d.ssq);
    double flux[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        const double(&n)[3] = nrm[f];
        if (nb[f] >= 0) {
            const double normal_len = fq(fa(fa(fm(n[0], n[0]), fm(n[1], n[1])), fm(n[2], n[2])));
            CfdDerived e;
            cfd_derive(w[f], e);
            // artificial viscosity
            const double factor = fm(fm(fm(-normal_len, smoothing_coefficient), double(0.5)),
                                     fa(fa(fa(speed_i, fq(e.ssq)), d.c), e.c));
            flux[0] = fa(flux[0], fm(factor, fs(v[0], w[f][0])));
            flux[4] = fa(flux[4], fm(factor, fs(v[4], w[f][4])));
            flux[1] = fa(flux[1], fm(factor, fs(v[1], w[f][1])));
            flux[2] = fa(flux[2], fm(factor, fs(v[2], w[f][2])));
            flux[3] = fa(flux[3], fm(factor, fs(v[3], w[f][3])));
            cfd_accumulate(n, &w[f][1], e.fmom, e.fe, v, d, flux);
        } else if (nb[f] == -1) {  // a wing boundary
            flux[1] = fa(flux[1], fm(n[0], d.p));
            flux[2] = fa(flux[2], fm(n[1], d.p));
            flux[3] = fa(flux[3], fm(n[2], d.p));
        } else if (nb[f] == -2) {  // a far field boundary
            const double ffm[3][3] = {{c.ff.momentum_x[0], c.ff.momentum_x[1], c.ff.momentum_x[2]},
                                      {c.ff.momentum_y[0], c.ff.momentum_y[1], c.ff.momentum_y[2]},
                                      {c.ff.momentum_z[0], c.ff.momentum_z[1], c.ff.momentum_z[2]}};
            const double ffe[3] = {c.ff.density_energy[0], c.ff.density_energy[1], c.ff.density_energy[2]};
            cfd_accumulate(n, &c.ff.variable[1], ffm, ffe, v, d, flux);
        }
    }

    // time_step (:356-362)
    const double factor = fdv(step, double(kCfdRk + 1 - j));
    double r[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = fa(o[k], fm(factor, flux[k]));
    if (vs == 1) {
        st_sc1_x4(&dst[at], make_uint4((uint32_t)__double2loint(r[0]), (uint32_t)__double2hiint(r[0]),
                                       (uint32_t)__double2loint(r[1]), (uint32_t)__double2hiint(r[1])));
        st_sc1_x4(&dst[at + 2], make_uint4((uint32_t)__double2loint(r[2]), (uint32_t)__double2hiint(r[2]),
                                           (uint32_t)__double2loint(r[3]), (uint32_t)__double2hiint(r[3])));
        st_agent(&dst[at + 4], r[4]);
    } else {
#pragma unroll
        for (int k = 0; k < 5; ++k) st_agent(&dst[at + k * vs], r[k]);
    }
}

// task (s, b): false (workgroup-uniform) where the task lies outside the plan
__device__ __forceinline__ bool cfd_task(const CfdCtx &c, int s, int b) {
    if (s < 0 || s >= c.stages || b < 0 || (long long)b * c.block >= c.nelr) return false;
    const int lo = b * c.block, hi = lo + c.block < c.nelr ? lo + c.block : c.nelr, j = s % kCfdRk;
    for (int i = lo + (int)threadIdx.x; i < hi; i += kCfdThreads) cfd_element(c, s, j, i);
    return true;
}

struct CfdKind : OnePromiseKind<CfdCtx> {
    static constexpr bool kSc1Payload = true;  // state, old and step_factors move by ld_agent / st_agent / st_sc1_x4 only
    __device__ static bool run_group(const CfdCtx &c, uint32_t, const uint32_t *pl, int) {
        if (!cfd_task(c, (int)pl[0], (int)pl[1])) {
            if (threadIdx.x == 0) dev_error(c.err, kErrBadTask);
            return false;
        }
        return true;
    }
};

__global__ __launch_bounds__(kCfdThreads) void k_cfd(CfdCtx c, DagView v) { run_dag_group<CfdKind>(c, v, nullptr); }

// the phases form: stage s, one workgroup per block
__global__ __launch_bounds__(kCfdThreads) void k_cfd_phase(CfdCtx c, int s) { (void)cfd_task(c, s, (int)blockIdx.x); }

int cfd_args(const char *who, bool ptrs_ok, int nel, const int *neighbours, int iterations, int &block, int form,
             CfdPlan &p) {
    if (!ptrs_ok) {
        set_error("%s: the arrays must not be NULL", who);
        return HCLIB_HIP_EINVAL;
    }
    std::string err;
    if (cfd_plan(nel, neighbours, iterations, block, form, p, err)) {
        set_error("%s: %s", who, err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    return HCLIB_HIP_OK;
}

}  // namespace
}  // namespace hx

using namespace hx;

extern "C" int hclib_hip_cfd_read_input(const char *path, double *areas, int *neighbours, double *normals,
                                        int64_t counts[2]) {
    if (!counts) {
        set_error("hclib_hip_cfd_read_input: counts must not be NULL");
        return HCLIB_HIP_EINVAL;
    }
    std::string err;
    int nel = 0, nelr = 0;
    if (cfd_read_input(path, (int)counts[0], areas, neighbours, normals, nel, nelr, err)) {
        set_error("hclib_hip_cfd_read_input: %s", err.c_str());
        return HCLIB_HIP_EINVAL;
    }
    counts[0] = nel;
    counts[1] = nelr;
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_cfd_bounds(int nel, const int *neighbours, int iterations, int block, uint64_t out[6]) {
    CfdPlan p;
    HX_TRY(cfd_args("hclib_hip_cfd_bounds", neighbours && out, nel, neighbours, iterations, block, HCLIB_HIP_CFD_DAG, p));
    out[0] = p.tasks;
    out[1] = p.awaits;
    out[2] = p.stages;
    out[3] = p.max_waiters;
    out[4] = p.arena_bytes;
    out[5] = p.bytes_moved;
    return HCLIB_HIP_OK;
}

extern "C" int hclib_hip_cfd(int nel, const double *areas, const int *neighbours, const double *normals,
                             const double *variables0, int iterations, int block, int form, double *variables,
                             hclib_hip_cfd_result_t *result) {
    // argument errors first, before the device is touched
    CfdPlan p;
    HX_TRY(cfd_args("hclib_hip_cfd", areas && neighbours && normals && variables, nel, neighbours, iterations, block, form,
                    p));
    const size_t n = (size_t)p.nelr;
    CfdCtx c;
    cfd_far_field(c.ff);
    // the initial state: the caller's, or the far field everywhere (initialize_variables, :127-130)
    std::vector<double> init;
    if (!variables0) {
        init.resize(n * kCfdNvar);
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < kCfdNvar; ++k) init[i * kCfdNvar + k] = c.ff.variable[k];
        variables0 = init.data();
    }
    if (result) {
        memset(result, 0, sizeof(*result));
        result->stages = p.stages;
        result->bytes_moved = p.bytes_moved;
        result->block = block;
        result->form = form;
    }
    HX_TRY(ensure_device());
    Module &m = mod();
    if (iterations == 0) {  // nothing to launch
        memmove(variables, variables0, n * kCfdNvar * sizeof(double));
        return HCLIB_HIP_OK;
    }

    // (HCLIB_HIP_CFD_LAYOUT: for measurements) 1: an array per variable on 256-byte lines; 0: 8 doubles per element
    const bool soa = env_int("HCLIB_HIP_CFD_LAYOUT", 1) != 0;
    const size_t pitch = cfd_pitch(n);
    c.es = soa ? 1 : (size_t)kCfdStride;
    c.vs = soa ? pitch : 1;
    const size_t state_bytes = cfd_up256((soa ? 5 * pitch : n * kCfdStride) * 8);
    const size_t o_nbs = cfd_up256(n * 8), o_nrm = o_nbs + cfd_up256(n * kCfdNnb * 4);
    const size_t o_v0 = o_nrm + cfd_up256(n * kCfdNnb * kCfdNdim * 8), o_v1 = o_v0 + state_bytes, o_old = o_v1 + state_bytes;
    const size_t o_sf = o_old + state_bytes, bytes = o_sf + cfd_up256(n * 8);
    char *d = nullptr;
    if (const int rc = arena_reserve(kArenaCfd, bytes, "hclib_hip_cfd", (void **)&d)) {
        set_error("hclib_hip_cfd: hipMalloc(%zu) failed (%d elements: the mesh, two states, old and the step factors)", bytes,
                  p.nelr);
        return rc;
    }
    // the state in the device layout
    std::vector<double> h0(state_bytes / 8, 0.0);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < kCfdNvar; ++k) h0[i * c.es + k * c.vs] = variables0[i * kCfdNvar + k];
    // (the host arrays outlive the copies: every path below synchronises the stream)
    HX_HIP(hipMemcpyAsync(d, areas, n * 8, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + o_nbs, neighbours, n * kCfdNnb * 4, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + o_nrm, normals, n * kCfdNnb * kCfdNdim * 8, hipMemcpyHostToDevice, m.stream));
    HX_HIP(hipMemcpyAsync(d + o_v0, h0.data(), state_bytes, hipMemcpyHostToDevice, m.stream));

    c.areas = (const double *)d;
    c.nbs = (const int *)(d + o_nbs);
    c.normals = (const double *)(d + o_nrm);
    c.var[0] = (double *)(d + o_v0);
    c.var[1] = (double *)(d + o_v1);
    c.old = (double *)(d + o_old);
    c.sf = (double *)(d + o_sf);
    c.err = nullptr;
    c.nelr = p.nelr;
    c.block = block;
    c.stages = (int)p.stages;

    hclib_hip_dag_stats_t st{};
    int rc = HCLIB_HIP_OK;
    if (form == HCLIB_HIP_CFD_DAG) {
        VersionGraph g;
        cfd_graph(p, g);
        // workgroups per CU: what the kernel's registers leave room for, at most 4 (HCLIB_HIP_CFD_WGS_PER_CU: for measurements)
        int fit = 1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, (const void *)k_cfd, kCfdThreads, 0) != hipSuccess || fit < 1)
            fit = 1;
        int wgs = env_int("HCLIB_HIP_CFD_WGS_PER_CU", 4);
        wgs = wgs < 1 ? 1 : (wgs > 8 ? 8 : wgs);
        if (wgs > fit) wgs = fit;
        rc = launch_dag_group(g, wgs, (const void *)k_cfd, kCfdThreads, "hclib_hip_cfd", &st,
                              [&](int grid, const DagView &v) {
                                  c.err = v.err;
                                  hipLaunchKernelGGL(k_cfd, dim3(grid), dim3(kCfdThreads), 0, m.stream, c, v);
                              });
    } else {
        rc = hip_check(hipEventRecord(m.ev0, m.stream), "hipEventRecord");
        for (int s = 0; rc == HCLIB_HIP_OK && s < (int)p.stages; ++s) {
            hipLaunchKernelGGL(k_cfd_phase, dim3(p.nblocks), dim3(kCfdThreads), 0, m.stream, c, s);
            rc = hip_check(hipGetLastError(), "hclib_hip_cfd: the launch of a stage");
        }
        if (rc == HCLIB_HIP_OK) rc = hip_check(hipEventRecord(m.ev1, m.stream), "hipEventRecord");
        const int rc_sync = hip_check(hipStreamSynchronize(m.stream), "hipStreamSynchronize");
        rc = rc ? rc : rc_sync;
        if (rc == HCLIB_HIP_OK) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, m.ev0, m.ev1);
            st.kernel_ms = ms;
            st.tasks = p.tasks;  // a workgroup per (stage, block); no promises
        }
    }
    if (result) {
        result->tasks = st.tasks;
        result->puts = st.puts;
        result->releases = st.releases;
        result->kernel_ms = st.kernel_ms;
        if (st.kernel_ms > 0) result->elements_per_s = (double)n * (double)p.stages / (st.kernel_ms * 1e-3);
    }
    if (rc) return rc;
    std::vector<double> h1(state_bytes / 8);
    HX_HIP(hipMemcpy(h1.data(), p.stages & 1 ? d + o_v1 : d + o_v0, state_bytes, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < kCfdNvar; ++k) variables[i * kCfdNvar + k] = h1[i * c.es + k * c.vs];
    return HCLIB_HIP_OK;
}
