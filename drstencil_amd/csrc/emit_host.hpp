// emit_host.hpp -- the text of an emitted file that is not the tuned kernel: the gold kernel (reference: codegen.hpp:637-660), the
// ring-fill (wrap) kernel of the non-fixed boundaries, the plugin entry points with the info JSON, and the two host programs (the reference's harness,
// codegen.hpp:547-635, and the N-GPU launcher of --gpus N).  Free functions of the const plan and the Schedule: none of them sees
// the kernel emitter's state.  HipEmitter::source() (emit_hip.hpp) concatenates the pieces.
#pragma once
#include <fstream>
#include <sstream>
#include <string>
#include "schedule.hpp"

namespace drs {

// ---- what the two host programs share
inline constexpr const char *kCheckErrorDef =
    "static void check_error (const char* message) {\n    hipError_t error = hipGetLastError ();\n    if (error != hipSuccess) {\n"
    "        printf (\"HIP error : %s, %s\\n\", message, hipGetErrorString (error));\n        exit(-1);\n    }\n}\n\n";
inline std::string interior_expr(const KernelPlan &p) {
    return p.ndim == 3 ? "(double)(L - 2 * Halo) * (M - 2 * Halo) * (N - 2 * Halo)" : "(double)(M - 2 * Halo) * (N - 2 * Halo)";
}
// RMS error of two host arrays over the outermost range `outer` ("a, b, first, one past the last") and the interior of the rest
inline std::string check_call(const KernelPlan &p, const std::string &outer) {
    return p.ndim == 3 ? "checkError3D (M, N, " + outer + ", Halo, M-Halo, Halo, N-Halo)" : "checkError2D (N, " + outer + ", Halo, N-Halo)";
}

// ---- the launch interface (plan.hpp: LaunchAbi) as text.  res is the one array a launch writes
inline std::string slot_type(int i, const char *elem) { return std::string(i == SLOT_RES ? "" : "const ") + elem + "*"; }
// the arrays the kernel takes (the gold kernel: no res), as the tail of dr_<name>'s / gold_<name>'s parameter list ...
inline std::string kernel_params(const LaunchAbi &abi, bool gold) {
    std::string t;
    for (int i = 0; i < NSLOTS; i++) if (abi.takes[i] && !(gold && i == SLOT_RES)) t += ", " + slot_type(i, "real_t") + " __restrict__ d_" + kSlotName[i];
    return t;
}
// ... and as the tail of its argument list inside an entry point
inline std::string kernel_args(const LaunchAbi &abi, bool gold) {
    std::string t;
    for (int i = 0; i < NSLOTS; i++) if (abi.takes[i] && !(gold && i == SLOT_RES)) t += ", (" + slot_type(i, "real_t") + ")" + kSlotName[i];
    return t;
}

// ---- gold kernel (codegen.hpp:637-660): one lane per point, interior guard, same sum
inline std::string gold_kernel(const KernelPlan &p) {
    std::ostringstream g;
    g << "// naive reference kernel: the verification arithmetic (same term order, same FMA chain)\n";
    g << "extern \"C\" __global__ void gold_" << p.name << " (const real_t* __restrict__ d_in, real_t* __restrict__ d_out" << kernel_params(LaunchAbi(p), true) << ")\n{\n";
    g << "    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);\n";
    g << "    const int j = (int)(blockIdx.y * blockDim.y + threadIdx.y);\n";
    if (p.ndim == 3) g << "    const int k = (int)(blockIdx.z * blockDim.z + threadIdx.z);\n";
    std::string guard = p.ndim == 3 ? "k >= Halo && k < L - Halo && j >= Halo && j < M - Halo && i >= Halo && i < N - Halo"
                                    : "j >= Halo && j < M - Halo && i >= Halo && i < N - Halo";
    g << "    if (" << guard << ") {\n";
    g << "        const real_t* c = d_in + " << (p.ndim == 3 ? "((long)k * M + j) * N + i" : "(long)j * N + i") << ";\n";
    bool first = true;
    const std::string gidx = p.ndim == 3 ? "((long)k * M + j) * N + i" : "(long)j * N + i";
    // --varcoef: tap t's coefficient is the value of grid t at this cell, in the constant's place
    if (p.varcoef) g << "        const real_t* a = d_coef + " << gidx << ";\n";
    int tap = 0;
    // taps are stored in role order; recover (k,j,i) offsets
    for (auto &t : p.gtaps) {
        long off;
        if (p.ndim == 3) off = ((long)t.ds * p.M + t.dy) * p.N + t.dx;
        else if (p.has_y) off = (long)t.dy * p.N + t.dx;
        else off = (long)t.ds * p.N + t.dx;
        const std::string cf = p.varcoef ? "a[" + std::to_string(tap) + "L * DRS_COEF_GRID]" : "(real_t)(" + t.coef + ")";
        if (first) g << "        real_t t = " << cf << " * c[" << off << "L];\n";
        else g << "        t = " << (p.fp32 ? "__builtin_fmaf" : "__builtin_fma") << "(" << cf << ", c[" << off << "L], t);\n";
        first = false;
        tap++;
    }
    if (p.scale) {       // explicit statements, in the sweep's order, each a rounded operation of its own: w *, [C * in +,] [- old,] [+ src,] [select]
        g << "        t = d_scale[" << gidx << "] * t;\n";
        if (p.centre_term()) g << "        { const real_t u = (real_t)(" << p.scale_centre << ") * c[0]; t = u + t; }\n";
        if (p.second_order) g << "        t = t - d_out[" << gidx << "];\n";
        if (p.source) g << "        t = t + d_src[" << gidx << "];\n";
        if (p.dirichlet) g << "        { const real_t f = d_fix[" << gidx << "]; t = (f != f) ? t : f; }\n";
        g << "        d_out[" << gidx << "] = t;\n";
    } else if (p.dirichlet) {   // explicit statements, in the sweep's order; the last one is a select, never arithmetic: a held cell receives fix bit for bit
        if (p.second_order) g << "        t = t - d_out[" << gidx << "];\n";
        if (p.source) g << "        t = t + d_src[" << gidx << "];\n";
        g << "        const real_t f = d_fix[" << gidx << "];\n";
        g << "        d_out[" << gidx << "] = (f != f) ? t : f;\n";
    } else if (p.source) {      // explicit statements: each a rounded operation of its own, in this order
        if (p.second_order) g << "        t = t - d_out[" << gidx << "];\n";
        g << "        d_out[" << gidx << "] = t + d_src[" << gidx << "];\n";
    } else if (p.second_order) g << "        d_out[" << gidx << "] = t - d_out[" << gidx << "];\n";
    else g << "        d_out[" << gidx << "] = t;\n";
    g << "    }\n}\n\n";
    return g.str();
}

// ---- non-fixed boundaries (--boundary periodic | reflect, --boundary-z / -y / -x) ---------------------------------------------------
// The ring fill.  Each axis maps a ring coordinate to an interior one (periodic: one period away; reflect: mirrored about the face between
// ring and interior; fixed: the identity, and that axis has no ring to fill).  Lanes [0, ghost rows * accesses per row): the ghost rows --
// rows (k, j) with k or j in the ring of a non-fixed axis -- each copied whole from row (map_z(k), map_y(j)), its x-ring columns mapped inside
// the lane's own vector (one lane writes every element of a destination vector; with x fixed they are copied straight).  Then, unless x is
// fixed, one lane per side of every other row: its Halo x ghosts.  A source's non-fixed coordinates are all interior and every destination
// has a coordinate in the ring of a non-fixed axis, so no source is a destination; every destination has one writer: no ordering inside
// the launch.
inline long wrap_planes(const KernelPlan &p) { return p.ndim == 3 ? p.L : 1; }
inline long wrap_zhalo(const KernelPlan &p) { return p.ndim == 3 && p.bmode[0] != FIXED ? p.halo : 0; }
inline long wrap_yhalo(const KernelPlan &p) { return p.bmode[1] != FIXED ? p.halo : 0; }
inline int wrap_vl(const KernelPlan &p) { return ((long)p.N * (p.fp32 ? 4 : 8)) % 16 == 0 ? 16 / (p.fp32 ? 4 : 8) : 1; }   // 16-byte vectors when rows stay aligned
inline long wrap_ghost_rows(const KernelPlan &p) { return 2 * wrap_zhalo(p) * p.M + (wrap_planes(p) - 2 * wrap_zhalo(p)) * 2 * wrap_yhalo(p); }
inline long wrap_sides(const KernelPlan &p) { return p.bmode[2] != FIXED ? (wrap_planes(p) - 2 * wrap_zhalo(p)) * (p.M - 2 * wrap_yhalo(p)) * 2 : 0; }
inline long wrap_grid(const KernelPlan &p) { return (wrap_ghost_rows(p) * (p.N / wrap_vl(p)) + wrap_sides(p) + 255) / 256; }
inline std::string wrap_kernel(const KernelPlan &p) {
    std::ostringstream w;
    const int vl = wrap_vl(p);
    const int mz = p.bmode[0], my = p.bmode[1], mx = p.bmode[2];
    const bool any_reflect = mz == REFLECT || my == REFLECT || mx == REFLECT;
    // a coordinate's map as emitted: the helper of the axis's mode; a fixed y or x coordinate stands for itself (z: a ring of width DRS_WHZ = 0)
    auto map = [](int mode, const std::string &x, const char *n, const char *h) {
        return mode == FIXED ? x : std::string(mode == REFLECT ? "drs_mirror(" : "drs_wrap(") + x + ", " + n + ", " + h + ")";
    };
    const std::string map_z = map(mz == REFLECT ? REFLECT : PERIODIC, "k", "DRS_WL", "DRS_WHZ"), map_y = map(my, "j", "M", "Halo");
    const std::string vec_kind = vl > 1 ? "16-byte vectors" : "elements (N * sizeof(real_t) is not a multiple of 16)";
    if (p.periodic)
        w << "// ---- periodic boundaries: wrap_" << p.name << "(a) fills a's ring of width Halo with the periodic images of a's interior (period\n"
             "// dim - 2 Halo; the ghost at x takes x + P below Halo and x - P from dim - Halo on, each coordinate wrapped on its own).  Every ring\n"
             "// element is written once, by one lane, from an interior element: one launch, no barrier.  Ghost rows (z-ghost planes, y-ghost rows)\n"
             "// are whole-row copies in " << vec_kind << ", then one lane per side of every interior row writes\n// its Halo x ghosts.  64-bit offsets throughout.\n";
    else {
        w << "// ---- boundaries (" << (p.ndim == 3 ? std::string("z ") + boundary_mode_name(mz) + ", " : std::string()) << "y " << boundary_mode_name(my) << ", x "
          << boundary_mode_name(mx) << "): wrap_" << p.name << "(a) fills a's ring of width Halo on the non-fixed axes from a's interior.  A ring\n"
             "// coordinate c of a periodic axis takes c + P below Halo and c - P from dim - Halo on (P = dim - 2 Halo); of a reflecting axis 2 Halo - 1 - c\n"
             "// and 2 (dim - Halo) - 1 - c (the zero-flux mirror about the face between ring and interior); a fixed axis keeps c, and its ring is never\n"
             "// written.  A cell is filled iff a coordinate of it lies in the ring of a non-fixed axis, once, by one lane, from the cell with every\n"
             "// coordinate mapped on its own: one launch, no barrier.  Ghost rows (k or j in such a ring) are whole-row copies in " << vec_kind << ";\n"
             "// " << (mx != FIXED ? "then one lane per side of every other row writes its Halo x ghosts" : "x is fixed: no other row is touched") << ".  64-bit offsets throughout.\n";
    }
    w << "#define DRS_WL " << wrap_planes(p) << "L          // planes of the grid (1 in 2D)\n";
    w << "#define DRS_WHZ " << wrap_zhalo(p) << (p.periodic ? "L         // ghost planes per side (0 in 2D)\n" : "L         // ghost planes per side (0: z is fixed, or 2D)\n");
    w << "#define DRS_WNV " << p.N / vl << "L        // accesses per ghost row\n";
    w << "#define DRS_WROWS " << wrap_ghost_rows(p) << "L    // ghost rows\n";
    w << "#define DRS_WSIDES " << wrap_sides(p) << (p.periodic ? "L   // sides of the interior rows\n" : "L   // sides of the rows that are no ghost rows (0: x is fixed)\n");
    w << "#define DRS_WGRID " << wrap_grid(p) << "\n";
    if (vl > 1) w << "typedef real_t drs_wvec_t __attribute__((ext_vector_type(" << vl << ")));\n";
    w << "__device__ __forceinline__ long drs_wrap(long x, long n, long h) { return x < h ? x + (n - 2 * h) : (x >= n - h ? x - (n - 2 * h) : x); }\n";
    if (any_reflect) w << "__device__ __forceinline__ long drs_mirror(long x, long n, long h) { return x < h ? 2 * h - 1 - x : (x >= n - h ? 2 * (n - h) - 1 - x : x); }\n";
    w << "extern \"C\" __global__ void __launch_bounds__(256) wrap_" << p.name << " (real_t* __restrict__ a)\n{\n";
    w << "    const long t = (long)blockIdx.x * 256 + threadIdx.x;\n";
    w << "    if (t < DRS_WROWS * DRS_WNV) {\n";
    w << "        const long r = t / DRS_WNV, v = t - r * DRS_WNV;\n";
    w << "        long k, j;\n";
    if (my != FIXED) {
        w << "        if (r < 2 * DRS_WHZ * M) { const long q = r / M; j = r - q * M; k = q < DRS_WHZ ? q : DRS_WL - 2 * DRS_WHZ + q; }\n";
        w << "        else { const long e = r - 2 * DRS_WHZ * M, q = e / (2 * Halo), c = e - q * (2 * Halo); k = DRS_WHZ + q; j = c < Halo ? c : M - 2 * Halo + c; }\n";
    } else      // y is fixed: every ghost row lies in a z-ghost plane
        w << "        { const long q = r / M; j = r - q * M; k = q < DRS_WHZ ? q : DRS_WL - 2 * DRS_WHZ + q; }\n";
    w << "        real_t* d = a + (k * M + j) * N;\n";
    w << "        const real_t* s = a + (" << map_z << " * M + " << map_y << ") * N;\n";
    if (vl > 1) {
        w << "        const long x = v * " << vl << ";\n";
        if (mx != FIXED) {
            w << "        drs_wvec_t u;\n";
            w << "        if (x >= Halo && x + " << vl << " <= N - Halo) u = *(const drs_wvec_t*)(s + x);\n";
            w << "        else {\n";
            for (int e = 0; e < vl; e++) w << "            u[" << e << "] = s[" << map(mx, "x + " + std::to_string(e), "N", "Halo") << "];\n";
            w << "        }\n";
            w << "        *(drs_wvec_t*)(d + x) = u;\n";
        } else      // x is fixed: the source row's x-ring columns come along unchanged
            w << "        *(drs_wvec_t*)(d + x) = *(const drs_wvec_t*)(s + x);\n";
    } else {
        w << "        d[v] = s[" << map(mx, "v", "N", "Halo") << "];\n";
    }
    if (mx != FIXED) {
        const std::string rows = my != FIXED ? "(M - 2 * Halo)" : "M", y0 = my != FIXED ? "Halo + " : "";
        w << "    } else if (t < DRS_WROWS * DRS_WNV + DRS_WSIDES) {\n";
        w << "        const long q = t - DRS_WROWS * DRS_WNV, r = q >> 1, pl = r / " << rows << ";\n";
        w << "        real_t* row = a + ((DRS_WHZ + pl) * M + " << y0 << "(r - pl * " << rows << ")) * N;\n";
        if (mx == PERIODIC)
            w << "        const long x0 = (q & 1) ? N - Halo : 0, from = (q & 1) ? -(N - 2 * Halo) : (N - 2 * Halo);   // right side : left side\n";
        else
            w << "        const long x0 = (q & 1) ? N - Halo : 0, from = (q & 1) ? -Halo : Halo;   // right side : left side; the Halo interior cells next to the face\n";
        w << "        real_t g[Halo];\n";
        w << "#pragma unroll\n        for (int e = 0; e < Halo; e++) g[e] = row[x0 + from + e];\n";
        if (mx == PERIODIC) w << "#pragma unroll\n        for (int e = 0; e < Halo; e++) row[x0 + e] = g[e];\n";
        else w << "#pragma unroll\n        for (int e = 0; e < Halo; e++) row[x0 + e] = g[Halo - 1 - e];   // mirrored: reversed\n";
    }
    w << "    }\n}\n\n";
    return w.str();
}

inline std::string info_json(const Schedule &s) {
    const KernelPlan &p = s.p; const GenOptions &o = s.o;
    std::string j = sfmt("{\\\"name\\\":\\\"%s\\\",\\\"ndim\\\":%d,\\\"dtype\\\":\\\"%s\\\",\\\"L\\\":%d,\\\"M\\\":%d,\\\"N\\\":%d,\\\"iterations\\\":%d,"
                         "\\\"step\\\":%d,\\\"halo\\\":%d,\\\"dist\\\":%d,\\\"range\\\":%d,\\\"taps\\\":%zu,\\\"threads\\\":%d,\\\"grid\\\":%d,"
                         "\\\"lds_bytes\\\":%ld,\\\"unroll\\\":%d,\\\"lds_slots\\\":%d,\\\"stages\\\":%d,\\\"schedule\\\":\\\"%s\\\",\\\"resident_planes\\\":%d,\\\"carry\\\":%d,\\\"reg_demand\\\":%d,\\\"points_per_lane\\\":%d,\\\"stage\\\":\\\"%s\\\","
                         "\\\"arithmetic\\\":\\\"%s\\\",\\\"tolerance_horizon_iterations\\\":%d,\\\"drift_estimate\\\":%.4g,\\\"drift_per_launch\\\":%.4g,\\\"temporal_forced\\\":%d,\\\"order\\\":\\\"%s\\\",\\\"packed\\\":%d,\\\"pinned\\\":%d,\\\"out_skew_bytes\\\":%ld,\\\"placement_period_bytes\\\":%ld,"
                         "\\\"sn\\\":%d,\\\"tile_owned_cols\\\":%d,\\\"tile_owned_rows\\\":%d,\\\"tiles_x\\\":%d,\\\"tiles_y\\\":%d,\\\"stream_blocks\\\":%d,\\\"streams\\\":%d,\\\"valid\\\":%d}",
                         p.name.c_str(), p.ndim, p.fp32 ? "fp32" : "fp64", p.L, p.M, p.N, p.iterations, p.step, p.halo, p.dist, p.range,
                         p.taps.size(), p.NT, s.grid_size(), s.lds_bytes(), s.UN, s.NSLOT, p.stages,
                         p.stages > 1 ? "temporal" : s.scatter() ? "scatter" : s.carry() ? "reuse" : "window", s.scatter() ? 1 : s.resident_planes(), s.scatter() ? p.zh - p.zl : s.carry(), s.reg_demand(), p.RY * p.VX, p.dma ? "dma" : "reg",
                         p.reassociated ? "reassociated" : "gold-order", p.reassociated ? p.horizon_iterations : -1, p.drift_estimate, p.drift_per_launch, p.temporal_forced ? 1 : 0,
                         s.rows_order() ? "rows" : "taps", s.packed() ? 1 : 0, s.pin() ? 1 : 0, s.out_skew_bytes(), Schedule::kPlacementPeriod,
                         p.SN, p.OX, p.OY, p.NBX, p.NBY, p.NBS, p.has_s ? 1 : 0,
                         (o.debug_drop_barrier || o.debug_skip) ? 0 : 1 /* 0: a timing experiment with barriers removed -- its results are wrong by design */);
    if (p.second_order) j.insert(j.size() - 1, ",\\\"time_order\\\":2");
    if (p.source) j.insert(j.size() - 1, ",\\\"source\\\":1");
    if (p.dirichlet) j.insert(j.size() - 1, ",\\\"dirichlet\\\":1");
    if (p.scale) j.insert(j.size() - 1, sfmt(",\\\"scale\\\":1,\\\"scale_centre\\\":%s", p.centre_term() ? p.scale_centre.c_str() : "0"));
    if (p.varcoef) {
        // tap t of coef, as (k, j, i) offsets (k = 0 in 2D): the order of the gold sum
        std::string taps;
        for (auto &t : p.taps) {
            const int kk = p.ndim == 3 ? t.ds : 0, jj = p.ndim == 3 ? t.dy : p.has_y ? t.dy : t.ds;
            taps += sfmt("%s[%d,%d,%d]", taps.empty() ? "" : ",", kk, jj, t.dx);
        }
        j.insert(j.size() - 1, ",\\\"varcoef\\\":1,\\\"coef_taps\\\":[" + taps + "]");
    }
    if (p.residual) j.insert(j.size() - 1, sfmt(",\\\"residual\\\":\\\"max\\\",\\\"residual_elems\\\":%ld", s.residual_elems()));
    if (p.periodic) {
        const int H = p.halo;
        j.insert(j.size() - 1, p.ndim == 3 ? sfmt(",\\\"boundary\\\":\\\"periodic\\\",\\\"period\\\":[%d,%d,%d]", p.L - 2 * H, p.M - 2 * H, p.N - 2 * H)
                                           : sfmt(",\\\"boundary\\\":\\\"periodic\\\",\\\"period\\\":[%d,%d]", p.M - 2 * H, p.N - 2 * H));
    } else if (p.fills_ring()) {
        std::string axes;
        for (int a = p.ndim == 3 ? 0 : 1; a < 3; a++) axes += sfmt("%s\\\"%s\\\"", axes.empty() ? "" : ",", boundary_mode_name(p.bmode[a]));
        j.insert(j.size() - 1, sfmt(",\\\"boundary\\\":\\\"%s\\\",\\\"boundaries\\\":[%s]", p.all_axes(REFLECT) ? "reflect" : "mixed", axes.c_str()));
    }
    return j;
}

// ---- plugin entry points (used when the source is built with -DDRS_PLUGIN -shared): the sweep's, the pair's with --pair-launch 1, the gold
// kernel's and the info, with the names and signatures of the plan's LaunchAbi (plan.hpp)
inline std::string plugin_api(const Schedule &s) {
    const KernelPlan &p = s.p; const GenOptions &o = s.o;
    const LaunchAbi abi(p, o.pair_launch != 0);
    std::ostringstream a;
    a << "// ---- launch entry points: bound by libdrstencil_amd's runtime (dlopen) and used by main() below\n";
    if (p.fills_ring()) {
        a << "// " << joined(boundary_words(p.ndim, p.bmode)) << ": drs_plugin_wrap fills a's ring from a's interior; both launch entry points call it on `in` first (same stream)\n";
        a << "extern \"C\" int drs_plugin_wrap(void* a, hipStream_t stream)\n{\n";
        a << "    hipLaunchKernelGGL(wrap_" << p.name << ", dim3(DRS_WGRID), dim3(256), 0, stream, (real_t*)a);\n";
        a << "    return (int)hipGetLastError();\n}\n";
    }
    // an entry point's head: every slot of its signature is a parameter, and one the kernel does not take (the caller passes NULL) is unused
    auto head = [&](const std::string &symbol, bool gold) {
        a << "extern \"C\" int " << symbol << "(const void* in, void* out";
        for (int i = 0; i < NSLOTS; i++) if (abi.in_signature(i, gold)) a << ", " << slot_type(i, "void") << " " << kSlotName[i];
        a << ", hipStream_t stream)\n{\n";
        if (p.fills_ring()) a << "    if (int rc = drs_plugin_wrap((void*)in, stream)) return rc;\n";
        for (int i = 0; i < NSLOTS; i++) if (abi.in_signature(i, gold) && !abi.takes[i]) a << "    (void)" << kSlotName[i] << ";\n";
    };
    // the sweep; with --residual max it writes the DRS_GRID partials d_res[1 ..] and res_<name> folds them into d_res[0], on the same stream
    head(abi.sweep_symbol(), false);
    a << "    hipLaunchKernelGGL(dr_" << p.name << ", dim3(DRS_GRID), dim3(DRS_NTL), 0, stream, (const real_t*)in, (real_t*)out" << kernel_args(abi, false) << ");\n";
    if (p.residual) a << "    hipLaunchKernelGGL(res_" << p.name << ", dim3(1), dim3(256), 0, stream, (real_t*)res);\n";
    a << "    return (int)hipGetLastError();\n}\n";
    if (abi.pair) {
        a << "extern \"C\" int drs_plugin_launch_pair(const void* in0, void* out0, const void* in1, void* out1, hipStream_t stream)\n{\n";
        a << "    hipLaunchKernelGGL(dr2_" << p.name << ", dim3(DRS_GRID, 2), dim3(DRS_NTL), 0, stream, (const real_t*)in0, (real_t*)out0, (const real_t*)in1, (real_t*)out1);\n";
        a << "    return (int)hipGetLastError();\n}\n";
    }
    head(abi.gold_symbol(), true);
    if (p.ndim == 3) a << "    dim3 b(64, 2, 2), g((N + 63) / 64, (M + 1) / 2, (L + 1) / 2);\n";
    else a << "    dim3 b(64, 4, 1), g((N + 63) / 64, (M + 3) / 4, 1);\n";
    a << "    hipLaunchKernelGGL(gold_" << p.name << ", g, b, 0, stream, (const real_t*)in, (real_t*)out" << kernel_args(abi, true) << ");\n";
    a << "    return (int)hipGetLastError();\n}\n";
    a << "extern \"C\" const char* drs_plugin_info(void)\n{\n    return \"" << info_json(s) << "\";\n}\n\n";
    return a.str();
}

// ---- N-GPU host (--gpus N): launcher and ranks in one program, on the C ABI's drs_slab_* entry points -----------------------------
// The reference has no counterpart (single device; SURVEY.md section 5 sketches this layer).  The program forks one rank process per
// GPU BEFORE any HIP call (a process that has initialised HIP must not fork), hands the RCCL id from rank 0 to the others through
// pipes, and follows the reference's protocol on every rank's slab: fill (the whole grid's rand() sequence, the rank's planes of it),
// warm-up, timed ping-pong loop, [Perf] from the slowest rank, and with --check every rank's own planes against the gold kernel run
// WITHOUT exchange on a slab that is launches x Halo planes wider per cut face.
inline std::string c_escape(const std::string &t) {
    std::string r;
    for (char c : t) {
        if (c == '\\' || c == '"') { r += '\\'; r += c; }
        else if (c == '\n') r += "\\n";
        else if (c == '\r' || c == '\t') r += ' ';
        else r += c;
    }
    return r;
}
inline std::string slab_host_main(const Schedule &s, const std::string &stc_path) {
    const KernelPlan &p = s.p; const GenOptions &o = s.o;
    std::string spec;
    { std::ifstream f(stc_path); std::stringstream b; b << f.rdbuf(); spec = b.str(); }
    std::string opts;
    for (auto &a : o.slab_args) opts += "\"" + c_escape(a) + "\", ";
    std::string t = R"HOST(#ifndef DRS_PLUGIN
// ---- N-GPU host (--gpus @WORLD@): launcher and ranks in one program (one process per GPU, forked before any HIP call); build with
//      hipcc ... -I<repo>/include -I<repo>/drstencil_amd/csrc/support -L<repo>/drstencil_amd -ldrstencil_amd -Wl,-rpath,<repo>/drstencil_amd
// Failure handling: rank 0 is the launcher.  A rank that dies or leaves with an error at ANY point makes rank 0 end the others and exit 1
// (SIGCHLD), a wall-clock watchdog does the same after DRS_SLAB_TIMEOUT seconds (default 900; 0: none) with exit code 124, and the ranks
// never outlive rank 0 (PR_SET_PDEATHSIG) -- nobody is left waiting in ncclCommInitRank or in a send/recv for a rank that has gone.
// Not under a profiler: `rocprofv3 --pmc` initialises the GPU before main(), and a process that has initialised HIP must not fork or start
// hipcc.  Profile ONE rank instead: DRS_SLAB_REHEARSE=r/R DRS_NO_COMPILE=1 after a plain run has filled the kernel cache.
#include <errno.h>
#include <string.h>
#include <unistd.h>
#include <sys/wait.h>
#include <sys/prctl.h>
#include <signal.h>
#pragma push_macro("L")
#pragma push_macro("M")
#pragma push_macro("N")
#undef L
#undef M
#undef N
#include "drstencil_amd.h"      // (its prototypes name parameters L, M, N: this file's size macros step aside)
#pragma pop_macro("N")
#pragma pop_macro("M")
#pragma pop_macro("L")

#define DRS_WORLD @WORLD@
static const char drs_spec_text[] = "@SPEC@";
static const char *drs_opts[] = { @OPTS@NULL };
#define DRS_NOPTS @NOPTS@
extern char **environ;

// the spec travels inside the program; the library reads it from a file.  The files live in a directory of this process's own
// (mkdtemp) under STABLE names -- @NAME@.stc, @NAME@_view<planes>.stc: the kernel name, and with it the kernel-cache key, is the same
// in every run and on every rank, so only the first run compiles -- and are removed on every way out.
static char drs_dir[400], spec_path[512], view_path[512];
static pid_t kids[DRS_WORLD];
static volatile sig_atomic_t kid_gone[DRS_WORLD];
static volatile int kid_status[DRS_WORLD];

static void drs_cleanup (void) {                                // unlink / rmdir are async-signal-safe
    if (view_path[0]) (void)unlink (view_path);
    if (spec_path[0]) (void)unlink (spec_path);
    if (drs_dir[0]) (void)rmdir (drs_dir);
    view_path[0] = spec_path[0] = drs_dir[0] = 0;
}
static void drs_say (const char* m) { if (write (2, m, strlen (m)) < 0) { } }
static void drs_abort_all (int code) {                           // rank 0: end the other ranks, clean up, leave (async-signal-safe)
    for (int r = 1; r < DRS_WORLD; r++) if (kids[r] > 0 && !kid_gone[r]) (void)kill (kids[r], SIGTERM);
    drs_cleanup ();
    _exit (code);
}
static void drs_on_sigchld (int sig) {
    (void)sig;
    const int saved = errno;
    for (int r = 1; r < DRS_WORLD; r++) {
        if (kids[r] <= 0 || kid_gone[r]) continue;
        int st = 0;
        if (waitpid (kids[r], &st, WNOHANG) != kids[r]) continue;
        kid_gone[r] = 1; kid_status[r] = st;
        if (!WIFEXITED (st) || WEXITSTATUS (st) != 0) { drs_say ("drstencil: a rank process failed; ending the others\n"); drs_abort_all (1); }
    }
    errno = saved;
}
static void drs_on_sigalrm (int sig) { (void)sig; drs_say ("drstencil: watchdog (DRS_SLAB_TIMEOUT) expired; ending every rank\n"); drs_abort_all (124); }
static void drs_on_sigterm (int sig) { (void)sig; drs_cleanup (); _exit (143); }

static int drs_under_profiler (void) {
    const char* pre = getenv ("LD_PRELOAD");
    if (pre && (strstr (pre, "rocprof") || strstr (pre, "roctracer"))) return 1;
    for (char** e = environ; e && *e; e++) if (strncmp (*e, "ROCPROF_", 8) == 0 || strncmp (*e, "ROCPROFILER_", 12) == 0) return 1;
    return 0;
}

@CHECKERROR@// planes > 0: the outermost size (@KEY@) replaced (a slab view)
static int write_spec (char* path, size_t cap, long planes) {
    if (planes > 0) snprintf (path, cap, "%s/@NAME@_view%ld.stc", drs_dir, planes);
    else snprintf (path, cap, "%s/@NAME@.stc", drs_dir);
    FILE* f = fopen (path, "w");
    if (!f) { path[0] = 0; return -1; }
    const char* t = drs_spec_text;
    const char* at = NULL;
    if (planes > 0)
        for (const char* c = t; c[0] && c[1]; c++)
            if (c[0] == '@KEY@' && (c == t || c[-1] == ' ' || c[-1] == '\n') && c[1] == ' ') { at = c + 1; while (*at == ' ') at++; break; }
    if (at) {
        const char* end = at;
        while (*end >= '0' && *end <= '9') end++;
        fwrite (t, 1, (size_t)(at - t), f);
        fprintf (f, "%ld", planes);
        fputs (end, f);
    } else fputs (t, f);
    fclose (f);
    return 0;
}

// one byte from every rank to rank 0 and rank 0's verdict back: 1 only if everybody said 1
static int drs_barrier (int rank, int world, int rehearsing, int (*id_pipe)[2], int (*res_pipe)[2], unsigned char mine) {
    if (rehearsing || world <= 1) return mine;
    unsigned char all = mine;
    if (rank != 0) {
        if (write (res_pipe[rank][1], &mine, 1) != 1) return 0;
        if (read (id_pipe[rank][0], &all, 1) != 1) return 0;
        return all && mine;
    }
    for (int r = 1; r < world; r++) { unsigned char ok = 0; if (read (res_pipe[r][0], &ok, 1) != 1 || !ok) all = 0; }
    for (int r = 1; r < world; r++) if (write (id_pipe[r][1], &all, 1) != 1) all = 0;
    return all;
}

int main(int argc, char **argv)
{
    (void)argc; (void)argv;
    puts("Initiating ...");
    int world = DRS_WORLD, rank = 0, rehearse = 0;
    const char* rh = getenv ("DRS_SLAB_REHEARSE");          // "r/R": rank r of R alone on ONE GPU, its neighbours being itself (no fork)
    if (rh) { if (sscanf (rh, "%d/%d", &rank, &rehearse) != 2 || rank < 0 || rank >= rehearse) { puts ("DRS_SLAB_REHEARSE=r/R"); return 2; } world = 1; }
    else if (getenv ("DRS_SLAB_WORLD")) { world = atoi (getenv ("DRS_SLAB_WORLD")); if (world < 1 || world > DRS_WORLD) { puts ("DRS_SLAB_WORLD=1..N"); return 2; } }   // fewer ranks than compiled in
    if (world > 1 && drs_under_profiler ()) {
        puts ("drstencil: the forking N-GPU form does not run under a profiler (the GPU is initialised before main; a process that has initialised HIP must not fork):\n"
              "           profile one rank with DRS_SLAB_REHEARSE=r/R DRS_NO_COMPILE=1 after a plain run has filled the kernel cache");
        return 2;
    }
    const long DIM0 = @DIM0@;                                 // planes of the whole grid
    const size_t plane = @PLANE@;                             // elements per plane
    const size_t npoints = (size_t)DIM0 * plane;
    // the whole grid's input (common.hpp:9-32: one rand() sequence) is filled ONCE, before the fork: the ranks share its pages copy-on-write
    // and each copies only its own planes to its GPU
    real_t* h_in = getRandomArray<real_t> (npoints);
    int id_pipe[DRS_WORLD][2], res_pipe[DRS_WORLD][2];
    memset (kids, 0, sizeof kids);
    (void)signal (SIGPIPE, SIG_IGN);                         // a rank that has gone shows up as a failed write, not as a signal
    fflush (stdout);
    if (world > 1) {                                         // rank 0's view of the others: installed before the first fork, reset in the children
        struct sigaction sa;
        memset (&sa, 0, sizeof sa);
        sa.sa_flags = SA_RESTART;
        sa.sa_handler = drs_on_sigchld; (void)sigaction (SIGCHLD, &sa, NULL);
        sa.sa_handler = drs_on_sigalrm; (void)sigaction (SIGALRM, &sa, NULL);
    }
    for (int r = 1; r < world; r++) {                        // ranks 1 .. N-1: forked BEFORE any HIP call; the parent is rank 0
        if (pipe (id_pipe[r]) || pipe (res_pipe[r])) { perror ("pipe"); drs_abort_all (1); }
        const pid_t pid = fork ();
        if (pid < 0) { perror ("fork"); drs_abort_all (1); }
        if (pid == 0) {
            rank = r;
            (void)signal (SIGCHLD, SIG_DFL); (void)signal (SIGALRM, SIG_DFL);
            memset (kids, 0, sizeof kids);
            (void)prctl (PR_SET_PDEATHSIG, SIGTERM);          // a rank never outlives the launcher (rank 0)
            (void)close (id_pipe[r][1]); (void)close (res_pipe[r][0]);
            for (int q = 1; q < r; q++) { (void)close (id_pipe[q][1]); (void)close (res_pipe[q][0]); }   // the launcher's ends of the earlier ranks' pipes (it has closed the others: those numbers may be ours now)
            break;
        }
        kids[r] = pid;
        (void)close (id_pipe[r][0]); (void)close (res_pipe[r][1]);
    }
    (void)signal (SIGTERM, drs_on_sigterm);                  // ended by rank 0 (or, rank 0, from outside): the spec files go too
    {   // fault injection for the tests of the failure paths (tests/test_gpu_parity.py::test_emitted_n_gpu_host): a rank that dies / hangs early
        const char* fr = getenv ("DRS_SLAB_TEST_FAIL_RANK");
        const char* hr = getenv ("DRS_SLAB_TEST_HANG_RANK");
        if (fr && atoi (fr) == rank && rank > 0) { printf ("[rank %d] injected failure\n", rank); fflush (stdout); _exit (7); }
        if (hr && atoi (hr) == rank && rank > 0) for (;;) (void)pause ();
    }
    if (rank == 0 && world > 1) {
        const char* to = getenv ("DRS_SLAB_TIMEOUT");
        const int secs = to ? atoi (to) : 900;
        if (secs > 0) (void)alarm ((unsigned)secs);
    }
#define DRS_FAIL(...) do { printf (__VA_ARGS__); fflush (stdout); if (rank == 0 && world > 1) drs_abort_all (1); drs_cleanup (); exit (1); } while (0)
    {
        const char* dir = getenv ("TMPDIR") ? getenv ("TMPDIR") : "/tmp";
        snprintf (drs_dir, sizeof drs_dir, "%s/drs_@NAME@_XXXXXX", dir);
        if (!mkdtemp (drs_dir)) { drs_dir[0] = 0; DRS_FAIL ("[rank %d] cannot make a directory under %s\n", rank, dir); }
        (void)atexit (drs_cleanup);
    }
    if (write_spec (spec_path, sizeof spec_path, 0) != 0) DRS_FAIL ("[rank %d] cannot write the spec under %s\n", rank, drs_dir);
    const char* args[DRS_NOPTS + 1];
    for (int i = 0; i < DRS_NOPTS; i++) args[i] = drs_opts[i];
    args[DRS_NOPTS] = spec_path;
    char* log = NULL;
    // plan + view kernels (this may run hipcc): before the first HIP call of this process
    drs_slab* s = drs_slab_open (DRS_NOPTS + 1, args, 0, NULL, world, rank, 1, rehearse, NULL, &log);
    if (!s) DRS_FAIL ("[rank %d] drs_slab_open failed: %s\n", rank, log ? log : "");
    long p[8];                                               // lo, hi, z0, z1, Lloc, G, H, every: holds planes [lo, hi), owns [z0, z1)
    drs_slab_plan (s, p);
    const int launches_per_loop = Iterations > 0 ? 2 * ((Iterations + 2 * Step - 1) / (2 * Step)) : 0;
    long wlo = p[2] - (long)launches_per_loop * Halo, whi = p[3] + (long)launches_per_loop * Halo;
    if (wlo < 0) wlo = 0;
    if (whi > DIM0) whi = DIM0;
    drs_kernel* kgold = NULL;
#if @CHECK@
    if (!rh) {                                               // the gold kernel of the wider no-exchange slab (built before HIP is up, like the views)
        if (write_spec (view_path, sizeof view_path, whi - wlo) != 0) DRS_FAIL ("[rank %d] cannot write the view spec under %s\n", rank, drs_dir);
        args[DRS_NOPTS] = view_path;
        kgold = drs_kernel_build (DRS_NOPTS + 1, args, NULL, &log);
        args[DRS_NOPTS] = spec_path;
        if (!kgold) DRS_FAIL ("[rank %d] gold view kernel: %s\n", rank, log ? log : "");
    }
#endif
    // Handshake before anything collective: every rank tells rank 0 whether it has its GPU; only if all have does rank 0 make the RCCL id and
    // send it (flag byte 1 + id) -- otherwise flag 0 and everybody leaves (a rank waiting in ncclCommInitRank for a dead one would wait for ever)
    unsigned char msg[1 + DRS_SLAB_ID_BYTES];
    memset (msg, 0, sizeof msg);
    const unsigned char ready = hipSetDevice (rh ? 0 : rank) == hipSuccess ? 1 : 0;
    if (!ready) printf ("[rank %d] no GPU %d on this node\n", rank, rank);
    if (rank != 0 && !rh) {
        if (write (res_pipe[rank][1], &ready, 1) != 1) return 1;
        if (read (id_pipe[rank][0], msg, sizeof msg) != (ssize_t)sizeof msg || !msg[0] || !ready) { drs_cleanup (); return 0; }   // nothing is run: the verdict (exit code 1) is rank 0's to give
    } else {
        unsigned char all = ready;
        for (int r = 1; r < world; r++) { unsigned char ok = 0; if (read (res_pipe[r][0], &ok, 1) != 1 || !ok) all = 0; }
        if (all && drs_slab_unique_id (msg + 1) != 0) { puts ("no RCCL"); all = 0; }
        msg[0] = all;
        for (int r = 1; r < world; r++) if (write (id_pipe[r][1], msg, sizeof msg) != (ssize_t)sizeof msg) all = 0;
        if (!all) {
            sigset_t blk; sigemptyset (&blk); sigaddset (&blk, SIGCHLD); (void)sigprocmask (SIG_BLOCK, &blk, NULL);
            for (int r = 1; r < world; r++) if (kids[r] > 0 && !kid_gone[r]) { int status = 0; (void)waitpid (kids[r], &status, 0); kid_gone[r] = 1; }
            puts ("not every rank has a GPU (or RCCL is missing): nothing was run");
            return 1;
        }
    }
    // a rank whose connect fails leaves at once (rank 0 then ends the others: they may be inside ncclCommInitRank waiting for it)
    if (drs_slab_connect (s, msg + 1, NULL) != 0) DRS_FAIL ("[rank %d] connect failed: %s\n", rank, drs_slab_error (s));

    const size_t n = (size_t)p[4] * plane, nbytes = n * sizeof(real_t);
    // both slab arrays in one allocation, the output @SKEWMIB@ MiB (mod 64 MiB) behind the input (--out-skew)
    const size_t out_at = (nbytes + @PERIOD@UL - 1) / @PERIOD@UL * @PERIOD@UL + @SKEW@UL;
    char* arena = NULL;
    unsigned char have = hipMalloc (&arena, out_at + nbytes) == hipSuccess && arena ? 1 : 0;
    real_t *in = (real_t*)arena, *out = (real_t*)(arena + out_at);
    if (have) have = hipMemcpy (in, h_in + (size_t)p[0] * plane, nbytes, hipMemcpyHostToDevice) == hipSuccess && hipMemset (out, 0, nbytes) == hipSuccess;
    if (!have) { printf ("[rank %d] HIP error : failed to allocate or fill the slab (%zu bytes): %s\n", rank, out_at + nbytes, hipGetErrorString (hipGetLastError ())); fflush (stdout); }
    // second barrier: everybody is connected and has its memory -- or everybody leaves, nobody waits in a send/recv for a rank that gave up
    if (!drs_barrier (rank, world, rh != NULL, id_pipe, res_pipe, have)) {
        if (rank == 0) {
            puts ("not every rank could set up its slab: nothing was run");
            if (world > 1) drs_abort_all (1);
        }
        drs_cleanup ();
        return rank == 0 ? 1 : 0;
    }
    printf ("[rank %d of %d] planes [%ld, %ld) of %ld, owns [%ld, %ld): %s\n", rank, rh ? rehearse : world, p[0], p[1], DIM0, p[2], p[3], drs_slab_info (s));

    puts("GPU computing ...");
    for (int i = 0; i < 3; i++) if (drs_slab_run (s, in, out, Iterations) < 0) DRS_FAIL ("[rank %d] run failed: %s\n", rank, drs_slab_error (s));   // warm up
    if (drs_slab_sync (s) != 0) DRS_FAIL ("[rank %d] sync failed: %s\n", rank, drs_slab_error (s));
    hipEvent_t ev0, ev1;
    (void)hipEventCreate (&ev0); (void)hipEventCreate (&ev1);
    hipStream_t st = (hipStream_t)drs_slab_stream (s);
    (void)hipEventRecord (ev0, st);
    const int launches = drs_slab_run (s, in, out, Iterations);
    (void)hipEventRecord (ev1, st);
    if (launches < 0 || drs_slab_sync (s) != 0) DRS_FAIL ("[rank %d] run failed: %s\n", rank, drs_slab_error (s));
    check_error ("Kernel error");
    float ms = 0.f;
    (void)hipEventElapsedTime (&ms, ev0, ev1);
    double rms = 0.0;
#if @CHECK@
    if (kgold) {
        // one loop from the pristine input through the slab run, the same loop with the gold kernel and NO exchange on [wlo, whi): own planes must agree
        (void)hipMemcpy (in, h_in + (size_t)p[0] * plane, nbytes, hipMemcpyHostToDevice);
        (void)hipMemset (out, 0, nbytes);
        if (drs_slab_run (s, in, out, Iterations) < 0 || drs_slab_sync (s) != 0) DRS_FAIL ("[rank %d] run failed: %s\n", rank, drs_slab_error (s));
        const size_t wn = (size_t)(whi - wlo) * plane;
        real_t *g_in, *g_out;
        (void)hipMalloc (&g_in, wn * sizeof(real_t)); (void)hipMalloc (&g_out, wn * sizeof(real_t));
        check_error ("Failed to allocate device memory for the gold slab.\n");
        (void)hipMemcpy (g_in, h_in + (size_t)wlo * plane, wn * sizeof(real_t), hipMemcpyHostToDevice);
        (void)hipMemset (g_out, 0, wn * sizeof(real_t));
        if (drs_kernel_run (kgold, g_in, g_out, Iterations, 1, NULL) < 0) DRS_FAIL ("[rank %d] gold run failed\n", rank);
        (void)hipDeviceSynchronize ();
        const size_t own = (size_t)(p[3] - p[2]) * plane;
        real_t* h_own = new real_t[own];
        real_t* h_gold = new real_t[own];
        (void)hipMemcpy (h_own, in + (size_t)(p[2] - p[0]) * plane, own * sizeof(real_t), hipMemcpyDeviceToHost);
        (void)hipMemcpy (h_gold, g_in + (size_t)(p[2] - wlo) * plane, own * sizeof(real_t), hipMemcpyDeviceToHost);
        long t0 = Halo - p[2], t1 = (p[3] - p[2]) - (p[3] - (DIM0 - Halo));    // the frozen ring of the WHOLE grid is not compared
        if (t0 < 0) t0 = 0;
        if (t1 > p[3] - p[2]) t1 = p[3] - p[2];
        printf ("[rank %d] ", rank);
        rms = @CHECKCALL@;
        delete[] h_own; delete[] h_gold;
        (void)hipFree (g_in); (void)hipFree (g_out);
    }
#endif
    // results: the slowest rank's time (and the largest error) reach rank 0 through the pipes
    int rc = 0;
    if (rank != 0 && !rh) {
        double rec[2] = { (double)ms, rms };
        if (write (res_pipe[rank][1], rec, sizeof rec) != (ssize_t)sizeof rec) rc = 1;
    } else {
        double worst_ms = ms, worst_rms = rms;
        for (int r = 1; r < world; r++) {
            double rec[2];
            if (read (res_pipe[r][0], rec, sizeof rec) != (ssize_t)sizeof rec) { printf ("rank %d sent no result\n", r); rc = 1; continue; }
            if (rec[0] > worst_ms) worst_ms = rec[0];
            if (rec[1] > worst_rms) worst_rms = rec[1];
        }
        if (world > 1) {                                     // every rank has reported or gone: collect the exit codes (the handler may have some already)
            sigset_t blk; sigemptyset (&blk); sigaddset (&blk, SIGCHLD); (void)sigprocmask (SIG_BLOCK, &blk, NULL);
            (void)alarm (0);
            for (int r = 1; r < world; r++) {
                int status = kid_status[r];
                if (!kid_gone[r]) { if (waitpid (kids[r], &status, 0) < 0) status = -1; kid_gone[r] = 1; }
                if (status == -1 || !WIFEXITED (status) || WEXITSTATUS (status) != 0) rc = 1;
            }
        }
        puts("GPU finished computing.");
        printf("GPU computation time: %f ms\n", worst_ms);
        {
            const double share = rh ? 1.0 / rehearse : 1.0;           // a rehearsal is one rank's share of the work
            const double updates = (double)launches * Step * @INTERIOR@ * share;
            const double bytes = (double)launches * 2.0 * sizeof(real_t) * (double)npoints * share / (rh ? 1 : world);
            if (launches > 0 && worst_ms > 0.0) {
                printf("[Perf] %.3f GStencil/s on %d GPU(s)%s, %d launches\n", updates / (worst_ms * 1e-3) / 1e9, rh ? 1 : world, rh ? " (REHEARSAL of one rank)" : "", launches);
                printf("[Perf] achieved %.1f GB/s per GPU = %.1f %% of the MI355X HBM3E roofline (8000 GB/s)\n", bytes / (worst_ms * 1e-3) / 1e9, bytes / (worst_ms * 1e-3) / 8e12 * 100.0);
            }
        }
#if @CHECK@
        if (!rh) printf("[Test] RMS Error : %e\n", worst_rms);
        else puts("[Test] skipped: a rehearsal's neighbours are the rank itself");
#endif
    }
    delete[] h_in;
    (void)hipFree (arena);
    drs_slab_close (s);
    drs_cleanup ();
    return rc;
}
#endif
)HOST";
    auto rep = [&](const std::string &key, const std::string &val) {
        size_t at = 0;
        while ((at = t.find(key, at)) != std::string::npos) { t.replace(at, key.size(), val); at += val.size(); }
    };
    const bool d3 = p.ndim == 3;
    rep("@WORLD@", std::to_string(o.gpus));
    rep("@SPEC@", c_escape(spec));
    rep("@OPTS@", opts);
    rep("@NOPTS@", std::to_string(o.slab_args.size()));
    rep("@NAME@", p.name);
    rep("@KEY@", d3 ? "L" : "M");
    rep("@DIM0@", d3 ? "L" : "M");
    rep("@PLANE@", d3 ? "(size_t)M * N" : "(size_t)N");
    rep("@CHECK@", o.check ? "1" : "0");
    rep("@PERIOD@", std::to_string(Schedule::kPlacementPeriod));
    rep("@SKEW@", std::to_string(s.out_skew_bytes()));
    rep("@SKEWMIB@", std::to_string(s.out_skew_bytes() >> 20));
    rep("@INTERIOR@", interior_expr(p));
    rep("@CHECKCALL@", check_call(p, "h_own, h_gold, (int)t0, (int)t1"));
    rep("@CHECKERROR@", kCheckErrorDef);
    return t;
}

// ---- host harness (codegen.hpp:547-635): same protocol, HIP events, size_t sizes
inline std::string host_main(const Schedule &s) {
    const KernelPlan &p = s.p; const GenOptions &o = s.o;
    std::ostringstream h;
    std::string dims = p.ndim == 3 ? "(size_t)L * M * N" : "(size_t)M * N";
    h << "#ifndef DRS_PLUGIN\n";
    h << kCheckErrorDef;
    h << "int main(int argc, char **argv)\n{\n    (void)argc; (void)argv;\n    puts(\"Initiating ...\");\n";
    h << "    const size_t npoints = " << dims << ";\n    const size_t nbytes = sizeof(real_t) * npoints;\n";
    if (p.second_order) h << "    real_t* h_in = getRandomArray<real_t> (npoints);\n    real_t* h_out = getRandomArray<real_t> (npoints);   // time order 2: out holds u(t-1), input too (the rand() sequence continued)\n";
    else h << "    real_t* h_in = getRandomArray<real_t> (npoints);\n    real_t* h_out = getZeroArray<real_t> (npoints);\n";
    // --source: the third array continues the reference's rand() fill behind the arrays filled today; it lies behind the pair in the same arena
    // the entry points and what they are passed beside (in, out): every slot of the signature, NULL where the kernel takes no such array
    const LaunchAbi abi(p);
    const std::string launch = abi.sweep_symbol(), gold = abi.gold_symbol();
    auto slot_args = [&](bool gold_form) {
        std::string t;
        for (int i = 0; i < NSLOTS; i++)
            if (abi.in_signature(i, gold_form)) t += !abi.takes[i] ? ", NULL" : i == SLOT_SRC ? ", src" : std::string(", d_") + kSlotName[i];
        return t;
    };
    const std::string sarg = slot_args(false), gsarg = slot_args(true);       // the gold kernel computes no residual
    if (p.source) h << "    real_t* h_src = getRandomArray<real_t> (npoints);   // the source term (the rand() sequence continued)\n";
    h << "    // both arrays in ONE allocation, the output " << (s.out_skew_bytes() >> 20) << " MiB (mod " << (Schedule::kPlacementPeriod >> 20) << " MiB) behind the input: launch time depends on (out - in) mod 64 MiB (--out-skew)\n";
    h << "    const size_t out_at = (nbytes + " << Schedule::kPlacementPeriod - 1 << "UL) / " << Schedule::kPlacementPeriod << "UL * " << Schedule::kPlacementPeriod << "UL + " << s.out_skew_bytes() << "UL;\n";
    if (p.source)
        h << "    const size_t src_at = (out_at + nbytes + 255UL) / 256UL * 256UL;   // the source array behind the pair\n"
             "    char *arena;\n    (void)hipMalloc (&arena, src_at + nbytes);\n    check_error (\"Failed to allocate device memory for in, out and src.\\n\");\n"
             "    real_t *in = (real_t*)arena, *out = (real_t*)(arena + out_at);\n    const real_t *src = (const real_t*)(arena + src_at);\n"
             "    (void)hipMemcpy (in, h_in, nbytes, hipMemcpyHostToDevice);\n    (void)hipMemcpy (out, h_out, nbytes, hipMemcpyHostToDevice);\n"
             "    (void)hipMemcpy (arena + src_at, h_src, nbytes, hipMemcpyHostToDevice);\n\n";
    else
    h << "    char *arena;\n    (void)hipMalloc (&arena, out_at + nbytes);\n    check_error (\"Failed to allocate device memory for in and out.\\n\");\n"
         "    real_t *in = (real_t*)arena, *out = (real_t*)(arena + out_at);\n"
         "    (void)hipMemcpy (in, h_in, nbytes, hipMemcpyHostToDevice);\n    (void)hipMemcpy (out, h_out, nbytes, hipMemcpyHostToDevice);\n\n";
    if (p.dirichlet)
        // the array of held cells continues the rand() fill behind every other array: a cell whose value falls below 1/4 is held at that value,
        // every other cell is free (NaN).  An allocation of its own, so that --source's arena stays as it is
        h << "    real_t* h_fix = getRandomArray<real_t> (npoints);   // --dirichlet (the rand() sequence continued): held at its value where that is < 1/4, else free\n"
             "    for (size_t x = 0; x < npoints; x++) if (!(h_fix[x] < (real_t)0.25)) h_fix[x] = (real_t)__builtin_nan (\"\");\n"
             "    real_t *d_fix;\n    (void)hipMalloc (&d_fix, nbytes);\n    check_error (\"Failed to allocate device memory for fix.\\n\");\n"
             "    (void)hipMemcpy (d_fix, h_fix, nbytes, hipMemcpyHostToDevice);\n";
    if (p.scale)
        // the array of factors continues the rand() fill behind every other array, mapped into [0.5, 1): a contraction for every stencil whose
        // taps' magnitudes sum to at most 1.  An allocation of its own, so that the other arrays' places stay as they are
        h << "    real_t* h_scale = getRandomArray<real_t> (npoints);   // --scale (the rand() sequence continued): factors in [0.5, 1)\n"
             "    for (size_t x = 0; x < npoints; x++) h_scale[x] = (real_t)0.5 + (real_t)0.5 * h_scale[x];\n"
             "    real_t *d_scale;\n    (void)hipMalloc (&d_scale, nbytes);\n    check_error (\"Failed to allocate device memory for scale.\\n\");\n"
             "    (void)hipMemcpy (d_scale, h_scale, nbytes, hipMemcpyHostToDevice);\n";
    if (p.varcoef)
        // the coefficient grids continue the rand() fill behind every other array, mapped into [0.5, 1) / T: the magnitudes of a cell's T
        // coefficients sum to less than 1, so iterating stays finite.  An allocation of its own, so that the other arrays' places stay as they are
        h << "    const size_t ncoef = " << p.taps.size() << "UL * npoints;   // --varcoef: " << p.taps.size() << " grids, tap t's at t * npoints\n"
             "    real_t* h_coef = getRandomArray<real_t> (ncoef);   // (the rand() sequence continued): coefficients in [0.5, 1) / " << p.taps.size() << "\n"
             "    for (size_t x = 0; x < ncoef; x++) h_coef[x] = ((real_t)0.5 + (real_t)0.5 * h_coef[x]) / (real_t)" << p.taps.size() << ";\n"
             "    real_t *d_coef;\n    (void)hipMalloc (&d_coef, sizeof(real_t) * ncoef);\n    check_error (\"Failed to allocate device memory for coef.\\n\");\n"
             "    (void)hipMemcpy (d_coef, h_coef, sizeof(real_t) * ncoef, hipMemcpyHostToDevice);\n";
    if (p.residual) h << "    real_t *d_res;   // --residual: [0] the last launch's max |out - in|, then one partial per workgroup; written whole by every launch\n"
                         "    (void)hipMalloc (&d_res, sizeof(real_t) * DRS_RES_ELEMS);\n    check_error (\"Failed to allocate device memory for the residual.\\n\");\n";
    h << "    puts(\"GPU computing ...\");\n\n    // warm up\n    for (int i = 0; i < 10; i ++) " << launch << " (in, out" << sarg << ", 0);\n\n";
    if (p.second_order)
        h << "    // time order 2: a launch reads its output, so the warm-up has advanced the state: both arrays start the timed (and checked) sequence afresh\n"
             "    (void)hipMemcpy (in, h_in, nbytes, hipMemcpyHostToDevice);\n    (void)hipMemcpy (out, h_out, nbytes, hipMemcpyHostToDevice);\n\n";
    h << "    hipEvent_t ev0, ev1;\n    (void)hipEventCreate (&ev0); (void)hipEventCreate (&ev1);\n    int launches = 0;\n    (void)hipEventRecord (ev0, 0);\n";
    h << "    for (int t = 0; t < Iterations; t += " << 2 * p.step << ") {\n        " << launch << " (in, out" << sarg << ", 0);\n        " << launch << " (out, in" << sarg << ", 0);\n        launches += 2;\n    }\n";
    h << "    (void)hipEventRecord (ev1, 0);\n    (void)hipDeviceSynchronize();\n    check_error (\"Kernel error\");\n    float ms = 0.f;\n    (void)hipEventElapsedTime (&ms, ev0, ev1);\n";
    h << "    puts(\"GPU finished computing.\");\n    printf(\"GPU computation time: %f ms\\n\", ms);\n";
    h << "    {\n        const double updates = (double)launches * Step * " << interior_expr(p) << ";\n"
         "        const double bytes = (double)launches * " << sfmt("%d.0", 2 + s.extra_streams() + (p.varcoef ? (int)p.taps.size() : 0)) << " * sizeof(real_t) * (double)npoints;\n"
         "        if (launches > 0 && ms > 0.f) {\n"
         "            printf(\"[Perf] %.3f GStencil/s, %d launches\\n\", updates / (ms * 1e-3) / 1e9, launches);\n"
         "            printf(\"[Perf] achieved %.1f GB/s = %.1f %% of the MI355X HBM3E roofline (8000 GB/s)\\n\", bytes / (ms * 1e-3) / 1e9, bytes / (ms * 1e-3) / 8e12 * 100.0);\n"
         "        }\n    }\n";
    if (p.residual)
        h << "    real_t h_res = (real_t)0;\n    (void)hipMemcpy (&h_res, d_res, sizeof(real_t), hipMemcpyDeviceToHost);\n    check_error (\"Failed to read the residual.\\n\");\n"
             "    printf(\"residual : %.17g\\n\", (double)h_res);\n";
    if (o.check) {
        h << "\n    // run the gold kernel and check error\n    puts (\"Checking error ...\");\n    real_t *g_in, *g_out;\n"
             "    (void)hipMalloc (&g_in, nbytes);\n    check_error (\"Failed to allocate device memory for g_in.\\n\");\n    (void)hipMemcpy (g_in, h_in, nbytes, hipMemcpyHostToDevice);\n"
             "    (void)hipMalloc (&g_out, nbytes);\n    check_error (\"Failed to allocate device memory for g_out.\\n\");\n    (void)hipMemcpy (g_out, h_out, nbytes, hipMemcpyHostToDevice);\n";
        h << "    for (int t = 0; t < Iterations; t += " << 2 * p.step << ") {\n        " << gold << " (g_in, g_out" << gsarg << ", 0);\n        " << gold << " (g_out, g_in" << gsarg << ", 0);\n    }\n";
        h << "    (void)hipDeviceSynchronize();\n    check_error (\"Kernel(gold) error\");\n    real_t* h_g_out = h_in;   // reuse the memory of the input array\n"
             "    (void)hipMemcpy (h_out, in, nbytes, hipMemcpyDeviceToHost);\n    (void)hipMemcpy (h_g_out, g_in, nbytes, hipMemcpyDeviceToHost);\n";
        h << "    double error = " << check_call(p, p.ndim == 3 ? "h_out, h_g_out, Halo, L-Halo" : "h_out, h_g_out, Halo, M-Halo") << ";\n";
        h << "    printf(\"[Test] RMS Error: %e\\n\", error);\n";
        if (p.residual) {
            // the last launch was (out -> in): its residual is max |in - out| over the interior of the arrays as they stand, which gold's arrays give on the host
            h << "    if (launches > 0) {\n        real_t* h_g_prev = new real_t[npoints];\n        (void)hipMemcpy (h_g_prev, g_out, nbytes, hipMemcpyDeviceToHost);\n"
                 "        real_t want = (real_t)0;\n";
            if (p.ndim == 3) h << "        for (int k = Halo; k < L - Halo; k++)\n";
            h << "        for (int j = Halo; j < M - Halo; j++)\n            for (int i = Halo; i < N - Halo; i++) {\n"
                 "                const size_t x = " << (p.ndim == 3 ? "((size_t)k * M + j) * N + i" : "(size_t)j * N + i") << ";\n"
                 "                const real_t diff = h_g_out[x] - h_g_prev[x];          // one rounded subtraction in the array's type\n"
                 "                const real_t d = diff < 0 ? -diff : diff;\n"
                 "                want = (d > want || d != d) ? d : want;\n            }\n"
                 "        const bool same = (want != want && h_res != h_res) || memcmp (&want, &h_res, sizeof(real_t)) == 0;\n"
                 "        if (!same) printf(\"Residual values differ : %.17g and %.17g\\n\", (double)want, (double)h_res);\n"
                 "        printf(\"[Test] Residual Error: %e\\n\", same ? 0.0 : (want != want || h_res != h_res) ? 1.0 / 0.0 : fabs ((double)want - (double)h_res));\n"
                 "        delete[] h_g_prev;\n    }\n";
        }
        h << "    (void)hipFree (g_in);\n    (void)hipFree (g_out);\n";
    }
    if (p.source) h << "\n    delete[] h_src;";
    if (p.residual) h << "\n    (void)hipFree (d_res);";
    if (p.dirichlet) h << "\n    delete[] h_fix;\n    (void)hipFree (d_fix);";
    if (p.scale) h << "\n    delete[] h_scale;\n    (void)hipFree (d_scale);";
    if (p.varcoef) h << "\n    delete[] h_coef;\n    (void)hipFree (d_coef);";
    h << "\n    delete[] h_in;\n    delete[] h_out;\n    (void)hipFree (arena);\n    return 0;\n}\n#endif\n";
    return h.str();
}

}  // namespace drs
