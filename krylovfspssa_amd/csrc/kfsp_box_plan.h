// Private: everything kfsp_set_matrix_box decides about a matrix-free box before it touches the device - the model's
// checks, the BoxDev descriptor, the single-factor BoxFast form and the host copy of its LDS image, which of the
// pencil (format 7), slab (format 8) and LDS-window (format 6) kernels the box may take and their geometry.  Plain
// inline host code without a context and without a HIP call: box_plan either fills a BoxPlan or names the refusal,
// and the entry point writes nothing into the context before it has succeeded.  tests/box_plan_check.cpp walks it
// under AddressSanitizer / UBSan.
#pragma once

#include "kfsp_internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace kfsp {

// A tiled order of the 128-row trips over a lexicographic box of n rows (ns species, dims fastest first): rows are cut
// below the slowest stride that is still at most 16 K rows (cut), r = hi * S_cut + lo; blocks of B = 1024 rows of lo; per
// block ALL lines hi back to back.  A row's +-S neighbours for the strides above the cut are then whole lines away - one
// line = B rows = 8 KB of x - instead of whole strides: 22^6 with the cut below species 4: the +-22^3 / 22^4 / 22^5
// neighbours sit 1 / 22 / 484 lines = 8 KB / 180 KB / 4 MB from the row in the order of the sweep.  Empty: keep the
// ascending order - fewer than three species, a cut stride under 2048 rows, or neither `force` nor a box beyond the
// caches.  Its one caller is the base-trip order of the pencil kernel (format 7, box_plan: the box is a plane,
// `force` comes from option "box_tile"); tests/box_tile_order_check.cpp calls it without a device.
inline std::vector<int32_t> box_tile_order(int ns, const int32_t *dims, int64_t n, bool force)
{
    std::vector<int32_t> out;
    const int64_t trips = (n + 127) / 128;
    if (ns < 3 || trips < 2 || trips > INT32_MAX) return out;
    int64_t stride = 1, smax = 1;
    int cut = -1;
    int64_t scut = 1;
    for (int s = 0; s < ns; ++s) {
        if (stride <= 16384 && s > 0) {
            cut = s;
            scut = stride;
        }
        smax = stride;
        stride *= dims[s];
    }
    const double mall = 256.0 * 1024 * 1024;
    const bool large = (double)n * 8.0 > mall && 8.0 * 2.0 * (double)smax * 8.0 > mall;
    if (cut < 1 || scut < 2048 || !(force || large)) return out;
    const int64_t B = 1024, nhi = (n + scut - 1) / scut;
    std::vector<std::pair<int64_t, int32_t>> key((size_t)trips);
    for (int64_t c = 0; c < trips; ++c) {
        const int64_t r = c * 128, lo = r % scut, hi = r / scut;
        key[(size_t)c] = {((lo / B) * nhi + hi) * scut + lo, (int32_t)c};
    }
    std::sort(key.begin(), key.end());
    out.resize((size_t)trips);
    for (int64_t c = 0; c < trips; ++c) out[(size_t)c] = key[(size_t)c].second;
    return out;
}

// option "box_tile" -> the `force` of the pencil kernel's base-trip order: -1 a plane beyond 4 MiB, 0 never (no order at
// all, whatever the size), 1 wherever box_tile_order has one to give
inline bool box_tile_wanted(int64_t tile) { return tile != 0; }
inline bool box_tile_force(int64_t tile, int64_t plane_rows) { return tile > 0 || (tile < 0 && plane_rows * 8 > (int64_t)(4 << 20)); }

// What the context keeps of a resident matrix-free box (kfsp_ctx::box): one assignment sets it, `= {}` clears it.
struct BoxGeom {
    bool on = false;              // the resident generator is a matrix-free box
    bool fast = false;            // the single-factor form (BoxFast) sits behind the tables
    // format 7 (pencils along the slowest species, kfsp_spmv_box.hip): eligible box, rows per plane, planes, base trips
    // (= ceil(rows per plane / 128)) and the length of their tiled order in d_pencil_order (0 entries: ascending)
    bool pencil = false, simple = false;
    int64_t plane_rows = 0, trips = 0, order_n = 0;
    int planes = 0;
    // format 8 (slabs): rows per line of the second-slowest species, lines, wavefronts per workgroup, workgroups per line set
    bool slab = false;
    int64_t line_rows = 0, lo_trips = 0;
    int lines = 0, waves = 0, groups = 0;
    size_t lds_bytes = 0;         // the table image a workgroup stages
    int reach = 0;                // rows of x staged in LDS on either side of a workgroup's 512 (format 6), 0: format 4
    BoxDev dev = {};              // the descriptor (host copy, passed as a kernel argument); pad = species * 16 + slots of
                                  // the fast form's instantiation
};

// the options and context facts the rules read
struct BoxPlanOpts {
    int64_t box_pencil = -1, box_slab_waves = 12, box_tile = -1, box_reach = 512;
    bool single = true;           // one rank and no communicator
};

struct BoxPlan {
    int64_t n = 0;                // states
    int64_t nnz = 0;              // entries of the whole generator, diagonal included
    BoxGeom g;
    BoxFast F;                    // (also the tail of `image`)
    std::vector<double> image;    // [0.0, 0.0][factor tables][species {sum, valid} tables][BoxFast], as it is uploaded
    std::vector<int32_t> order;   // the pencil kernel's base trips (box_tile_order), empty: ascending
};

// the checks on the arguments themselves, which kfsp_set_matrix_box makes before it forwards a group head's call
inline int box_plan_args(int32_t ns, const int32_t *dims, int32_t nr, const int32_t *stoich, const int32_t *ndep,
                         const int32_t *dep_species, const double *tables, const char **what)
{
    auto fail = [&](int code, const char *text) {
        *what = text;
        return code;
    };
    if (ns < 1 || ns > kBoxMaxS) return fail(-2, "1 <= ns <= 8");
    if (!dims) return fail(-3, "null dims");
    if (nr < 1 || nr > kBoxMaxR) return fail(-4, "1 <= nr <= 16");
    if (!stoich || !ndep || !dep_species) return fail(-5, "null reaction description");
    if (!tables) return fail(-8, "null tables");
    return 0;
}

// The seven model arguments of kfsp_set_matrix_box -> P, or the status code and text (*what) the entry point returns.
inline int box_plan(int32_t ns, const int32_t *dims, int32_t nr, const int32_t *stoich, const int32_t *ndep,
                    const int32_t *dep_species, const double *tables, const BoxPlanOpts &opt, BoxPlan &P, const char **what)
{
    auto fail = [&](int code, const char *text) {
        *what = text;
        return code;
    };
    if (int rc = box_plan_args(ns, dims, nr, stoich, ndep, dep_species, tables, what)) return rc;
    P = BoxPlan();
    int64_t n = 1, stride[kBoxMaxS];
    for (int s = 0; s < ns; ++s) {
        if (dims[s] < 1) return fail(-3, "dims must be positive");
        stride[s] = n;
        n *= dims[s];
        if (n > 2147483647LL - 512) return fail(-3, "box has more than 2^31 states");
    }
    if (n < 2) return fail(-3, "box has fewer than 2 states");
    P.n = n;
    // reactions sorted by the column offset of their entry (ascending, like the stored diagonals)
    struct R { int64_t delta; int k; };
    std::vector<R> order((size_t)nr);
    for (int k = 0; k < nr; ++k) {
        int64_t d = 0;
        for (int s = 0; s < ns; ++s) d -= (int64_t)stoich[(size_t)k * ns + s] * stride[s];
        order[(size_t)k] = R{d, k};
    }
    std::stable_sort(order.begin(), order.end(), [](const R &a, const R &b) { return a.delta < b.delta; });
    BoxGeom &G = P.g;
    BoxDev &B = G.dev;
    std::memset(&B, 0, sizeof(B));
    B.ns = ns;
    B.nr = nr;
    for (int s = 0; s < ns; ++s) {
        B.dims[s] = dims[s];
        B.inv_dim[s] = 1.0 / (double)dims[s];
    }
    // table offsets in the order the caller concatenated them: reaction by reaction, factor by factor
    std::vector<int32_t> toff((size_t)nr * kBoxMaxDep, 0);
    int64_t ntab = 0;
    for (int k = 0; k < nr; ++k) {
        if (ndep[k] < 1 || ndep[k] > kBoxMaxDep) return fail(-6, "1 <= ndep <= 3 factors per propensity");
        for (int i = 0; i < ndep[k]; ++i) {
            const int s = dep_species[(size_t)k * kBoxMaxDep + i];
            if (s < 0 || s >= ns) return fail(-7, "factor species out of range");
            toff[(size_t)k * kBoxMaxDep + i] = (int32_t)ntab;
            ntab += dims[s];
        }
    }
    const int head = kBoxImageHead;              // image = [0.0, 0.0][factor tables][fast form's species tables]
    if (head + ntab > 6000) return fail(-8, "factor tables exceed the 48 KB they may take in LDS");
    for (int p = 0; p < nr; ++p) {
        const int k = order[(size_t)p].k;
        B.delta[p] = (int32_t)order[(size_t)p].delta;
        B.ndep[p] = (int8_t)ndep[k];
        for (int i = 0; i < ndep[k]; ++i) {
            const int s = dep_species[(size_t)k * kBoxMaxDep + i];
            B.dep_s[p][i] = (int8_t)s;
            B.dep_nu[p][i] = (int8_t)stoich[(size_t)k * ns + s];
            B.dep_off[p][i] = head + toff[(size_t)k * kBoxMaxDep + i];
        }
        int nm = 0;
        for (int s = 0; s < ns; ++s) {
            const int v = stoich[(size_t)k * ns + s];
            if (v == 0) continue;
            if (nm == kBoxMaxDep) return fail(-5, "a reaction changes more than 3 species");
            if (v < -100 || v > 100) return fail(-5, "stoichiometry out of range");
            B.mov_s[p][nm] = (int8_t)s;
            B.mov_nu[p][nm] = (int8_t)v;
            B.mov_dim[p][nm] = dims[s];
            ++nm;
        }
        B.nmov[p] = (int8_t)nm;
        B.dorder[k] = p;                               // original reaction k sits at sorted position p
    }
    // single-factor fast form: every propensity one factor, no species changes by more than 2, at
    // most kBoxFastPer propensities per species, the entries of a row within 2^32 bytes of x
    BoxFast &F = P.F;
    std::memset(&F, 0, sizeof(F));
    bool fast = ns <= kBoxFastS;
    int per_species[kBoxMaxS] = {0};
    for (int k = 0; k < nr && fast; ++k) {
        fast = ndep[k] == 1;
        for (int s = 0; s < ns; ++s) fast = fast && std::abs(stoich[(size_t)k * ns + s]) <= 2;
        if (fast) fast = ++per_species[dep_species[(size_t)k * kBoxMaxDep]] <= kBoxFastPer;
    }
    const int64_t back = std::max<int64_t>(0, -order.front().delta), fwd = std::max<int64_t>(0, order.back().delta);
    if (back + fwd + 130 >= (1LL << 28)) fast = false;
    int per = 2, ns_inst = kBoxFastS;
    int64_t df_at[kBoxFastS] = {0};
    int64_t nimage = head + ntab;
    if (fast) {
        for (int s = 0; s < ns; ++s) per = std::max(per, per_species[s]);
        if (per > 2) per = kBoxFastPer;
        // instantiations (launch_spmv): 2, 3 or 6 species with 2 slots each, else 6 species with 4 slots
        ns_inst = (per == 2 && ns <= 2) ? 2 : (per == 2 && ns == 3) ? 3 : kBoxFastS;
        nimage += nimage & 1;
        for (int s = 0; s < ns_inst; ++s) {
            df_at[s] = nimage;
            nimage += 2 * (s < ns ? dims[s] : 1);
        }
        if (nimage > 8180) {                                  // 64 KB of LDS less the kernel's own few words
            fast = false;
            nimage = head + ntab;
        }
    }
    std::vector<double> &image = P.image;
    image.assign((size_t)nimage + (sizeof(BoxFast) + 7) / 8, 0.0);
    std::memcpy(image.data() + head, tables, (size_t)ntab * sizeof(double));
    if (fast) {
        F.ns = ns_inst;
        F.per = per;
        F.bias8 = (int32_t)(8 * back);
        for (int s = 0; s < kBoxFastS; ++s) {
            F.dims[s] = s < ns ? dims[s] : 1;                 // missing species: one population count, 0
            F.inv_dim[s] = 1.0 / (double)F.dims[s];
            F.df8[s] = (int32_t)(8 * df_at[s]);
        }
        struct DF { double dsum; uint32_t valid, pad; };
        static_assert(sizeof(DF) == 16, "layout of the kernel's BoxDF");
        int fill[kBoxFastS] = {0};
        int entry_k[kBoxFastS * kBoxFastPer];
        for (int e = 0; e < ns_inst * per; ++e) entry_k[e] = -1;
        for (int p = 0; p < nr; ++p) {                        // ascending column offset within a species
            const int k = order[(size_t)p].k;
            const int s = dep_species[(size_t)k * kBoxMaxDep];
            const int j = fill[s]++;
            F.koff8[s][j] = 8 * (head + toff[(size_t)k * kBoxMaxDep] - stoich[(size_t)k * ns + s]);
            F.delta8[s][j] = (int32_t)(8 * order[(size_t)p].delta);
            entry_k[s * per + j] = k;
        }
        for (int s = 0; s < ns_inst; ++s) {
            const int d = s < ns ? dims[s] : 1;
            DF *df = reinterpret_cast<DF *>(image.data() + df_at[s]);
            for (int i = 0; i < d; ++i) {
                double sum = 0.0;
                uint32_t valid = 0;
                for (int e = 0; e < ns_inst * per; ++e) {
                    const int k = entry_k[e];
                    if (k < 0) continue;                      // unused slot: never valid
                    const int v = s < ns ? stoich[(size_t)k * ns + s] : 0;   // source coordinate = i - v
                    if (i - v >= 0 && i - v < d) valid |= 1u << e;
                    if (e / per == s) sum += tables[(size_t)toff[(size_t)k * kBoxMaxDep] + i];
                }
                df[i] = DF{sum, valid, 0u};
            }
        }
        B.pad = ns_inst * 16 + per;
    }
    B.ntab = (int32_t)nimage;
    std::memcpy(image.data() + nimage, &F, sizeof(F));
    G.fast = fast;
    // Format 7 (pencils, kfsp_spmv_box.hip): the instantiation's species are the model's (no padding species), the slowest
    // species' own entries reach exactly one plane (or are unused slots), no other entry moves the slowest species, planes
    // have an even number of rows (16-byte pairs), one rank, and there are enough base trips to fill the chip.
    if (fast && ns >= 3 && ns == ns_inst && opt.single) {
        const int Ls = ns - 1;
        int64_t plane = 1;
        for (int s = 0; s < Ls; ++s) plane *= dims[s];
        // (1: also small boxes - tests.  Nothing else is required of the reactions: an entry that does not fit the register
        // scheme - it depends on the slowest species but moves another, or moves the slowest by two - is gathered from
        // memory as in format 4; entries of other species that move the slowest one get that species' valid bit per step)
        const bool ok = (plane % 2 == 0) && dims[Ls] >= 2 && ((plane + 127) / 128 >= 4096 || opt.box_pencil > 0);
        bool simple = true;
        for (int k = 0; k < nr; ++k)
            if (dep_species[(size_t)k * kBoxMaxDep] != Ls && stoich[(size_t)k * ns + Ls] != 0) simple = false;
        G.simple = simple;
        // Format 8 (slabs): additionally the lines of the second-slowest species have an even number of rows, there are at
        // least two of them, and at least 256 workgroups' worth of slabs (or the option insists)
        if (ok && ns >= 3) {
            int64_t line = 1;
            for (int s = 0; s < Ls - 1; ++s) line *= dims[s];
            const int lines = dims[Ls - 1];
            const int wmax = (int)std::max<int64_t>(1, std::min<int64_t>(12, opt.box_slab_waves));   // (<= 12 wavefronts per workgroup)
            const int groups = (lines + wmax - 1) / wmax, waves = (lines + groups - 1) / groups;
            const int64_t lo_trips = (line + 127) / 128;
            if (line % 2 == 0 && lines >= 2 && (lo_trips * groups >= 256 || opt.box_pencil == 2)) {
                G.slab = true;
                G.line_rows = line;
                G.lines = lines;
                G.groups = groups;
                G.waves = waves;
                G.lo_trips = lo_trips;
            }
        }
        if (ok) {
            G.pencil = true;
            G.plane_rows = plane;
            G.planes = dims[Ls];
            G.trips = (plane + 127) / 128;
            // the base trips in small tiles of the plane (box_tile_order on the plane's species; option "box_tile": 0 never,
            // 1 wherever there is such an order, -1 a plane beyond 4 MiB)
            if (box_tile_wanted(opt.box_tile)) P.order = box_tile_order(Ls, dims, plane, box_tile_force(opt.box_tile, plane));
            G.order_n = (int64_t)P.order.size();
        }
    }
    // format 6: the largest shift within box_reach rows decides how much of x a workgroup stages in LDS;
    // the windows must fit beside the table image in the 64 KB a workgroup gets without asking for more
    if (fast) {
        int64_t reach = 0;
        for (int p = 0; p < nr; ++p) {
            const int64_t d = std::llabs((long long)order[(size_t)p].delta);
            if (d <= opt.box_reach) reach = std::max(reach, d);
        }
        reach = (reach + 1) & ~(int64_t)1;
        const size_t need = (((size_t)nimage * 8 + 15) & ~(size_t)15) + 2 * (size_t)(512 + 2 * reach) * 8 + 256;
        if (reach > 0 && need <= 64 * 1024) G.reach = (int)reach;
    }
    G.lds_bytes = (size_t)nimage * sizeof(double);
    int64_t nnz = n;
    for (int k = 0; k < nr; ++k) {
        int64_t c = 1;
        for (int s = 0; s < ns; ++s) c *= std::max<int64_t>(0, dims[s] - std::abs(stoich[(size_t)k * ns + s]));
        nnz += c;
    }
    P.nnz = nnz;
    G.on = true;
    return 0;
}

}  // namespace kfsp
