/*
 * rt_lower.h -- host side, no HIP call: the second half of scene compilation.  rt_compile.h lowers a validated hittable
 * graph to a CompiledScene; lower_scene() below turns that into every array the device reads (step program, instance
 * visits, per-reference records with their tie and guard flags, leaf records, scan runs, FMat) and into the facts every
 * kernel-variant decision hangs on (SceneFacts: pick_trav, mega_variant and the wavefront plan of rt_select.h read
 * nothing else).  rtr_upload_scene only copies what comes out of here.  Included through rt_select.h / rt_context.h by the units of the C ABI: the megakernel
 * and wavefront units do not see it.
 */
#pragma once

#include "rt_compile.h"
#include "rt_machine.h" /* FVisit */

#include <functional>

/* what the library knows about the uploaded scene beyond rtr_scene_info: the context holds one, assigned whole */
struct SceneFacts {
    int fast_stack_words = 1;
    int walk_extra_words = 0; /* stack of a compiled subtree's box tree on top of the walk's own */
    bool lean_materials = false; /* only lambertian / diffuse_light with solid_color textures, only QuadLights */
    bool quad_lights_only = false;
    bool flat_scene = false; /* compiled scene without box trees and without tie-capable references */
    bool flat_guarded = false; /* a flat scene but for guarded references: RT_TRAV_FAST everywhere, RT_TRAV_FLAT_GUARD in the megakernel */
    /* a moving_sphere (its hit() writes no u,v: the record keeps those of an earlier, farther hit of the
     * reference's walk) carries a material that reads (u,v): only the reference-order walk reproduces that */
    bool uv_order_dependent = false;
    bool machine_ok = false; /* the compiled scene fits the position word of the traversal machine (rt_machine.h) */
    bool guarded_program = false; /* the step program holds guarded primitives (FStep kind 3) or media under wrappers: not a program of the machine */
    bool top_tree = false;  /* sub-scene 0 has a top tree: the per-lane instance walk (FSub) */
    bool needs_uv = false;  /* rtr_scene_info::needs_uv */
    bool pair_cast = false; /* DScene::pair_cast */
    int n_material_types = 0;
    int n_materials = 0;
    double t_lo = 0, t_hi = 0; /* the ray times the scene was compiled for (rt_compile.h: t_lo, t_hi) */
    bool camera_times_small = true; /* the uploaded camera passed the 2^60 test of DScene::shared_div */
};

struct LoweredScene {
    CompiledScene cs;            /* inst[] final: with scan runs */
    std::vector<FStep> steps;    /* cs.steps, or the default one-step program */
    std::vector<FVisit> visits;
    std::vector<rtr_node> prims; /* per reference: the node record with visiting order, exit code, guard words, tie flag */
    std::vector<FLeaf> leaves;
    std::vector<FMat> mats;
    std::vector<FFin> finish;    /* per reference, or empty: the scene gets none (build_finish) */
    SceneFacts facts;
    DScene ds; /* every member that is not a device pointer; the others, and the padding, zero */
};

namespace rtc {

/* the compiled scene and what rtr_scene_info says about it (rtr_validate_scene stops here) */
inline CompiledScene compile_validated(const rtr_scene_desc* s, rtr_scene_info& info) {
    CompiledScene cs = compile_scene(s, info.has_media != 0 || info.inverted_boxes != 0, info.has_media == 0 && info.inverted_boxes != 0);
    info.fast_ok = cs.ok;
    info.fast_instances = (int32_t)cs.inst.size();
    info.fast_refs = (int32_t)cs.ref.size();
    info.fast_stack_words = cs.stack_words;
    info.compiled_subtrees = cs.n_compiled_subtrees;
    info.program_steps = (int32_t)cs.steps.size();
    info.top_trees = 0;
    for (const FSub& sub : cs.subs) info.top_trees += sub.top_root >= 0;
    return cs;
}

/* the traversal machine of the wavefront stages always runs a step program: a scene without media is
 * the one-step program "sub-scene 0" */
inline std::vector<FStep> build_steps(const CompiledScene& cs) {
    std::vector<FStep> dev_steps = cs.steps;
    if (cs.ok && dev_steps.empty()) {
        FStep whole{};
        whole.kind = 0, whole.sub = 0;
        dev_steps.push_back(whole);
    }
    return dev_steps;
}

/* ... flattened into instance visits in execution order */
inline std::vector<FVisit> build_visits(const CompiledScene& cs, const std::vector<FStep>& dev_steps) {
    std::vector<FVisit> visits;
    for (size_t k = 0; k < dev_steps.size(); ++k) {
        const FStep& st = dev_steps[k];
        const FSub& sub = cs.subs[st.sub];
        const int first = (int)visits.size();
        for (int q = 0; q < sub.n_inst; ++q) {
            const FInst& I = cs.inst[sub.inst_first + q];
            FVisit v{};
            v.flags = (q == 0 ? FV_FIRST : 0) | (q == sub.n_inst - 1 ? FV_LAST : 0) | (st.kind != 0 ? FV_MEDIUM : 0) |
                      (sub.n_inst > RT_FAST_NO_BOX_MAX ? FV_BOXES : 0) | ((int)k >= cs.step_tail ? FV_TAIL : 0);
            v.step = (int32_t)k, v.inst = sub.inst_first + q, v.step_first = first;
            v.xf_first = I.xf_first, v.n_xf = I.n_xf, v.ref_first = I.ref_first, v.n_ref = I.n_ref;
            v.bvh_root = I.bvh_root, v.bound = I.bound;
            v.neg_inv_density = st.neg_inv_density;
            visits.push_back(v);
        }
    }
    return visits;
}

/* the node record of every reference: visiting order, exit-wrapper code and guard words (no tie flag yet) */
inline std::vector<rtr_node> build_prims(const rtr_scene_desc* s, const CompiledScene& cs) {
    std::vector<rtr_node> prims(cs.ref.size());
    for (size_t k = 0; k < cs.ref.size(); ++k) {
        prims[k] = s->nodes[cs.ref[k].node]; /* original records */
        prims[k].reserved = cs.ref[k].pad;      /* visiting order of the reference's walk */
        /* the wrappers above the reference as a code in f[9] (see RT_EXIT_LONG) */
        unsigned long long code = 0;
        bool fits = prims[k].type != RTR_NODE_MOVING_SPHERE && cs.ref[k].n_exit <= 31;
        for (int e = 0; e < cs.ref[k].n_exit && fits; ++e) {
            const int wt = s->nodes[cs.exits[cs.ref[k].exit_first + e]].type;
            code |= (unsigned long long)(wt == RTR_NODE_FLIP_FACE ? 2 : 1) << (2 * e);
        }
        if (!fits) code = RT_EXIT_LONG;
        if (prims[k].type != RTR_NODE_MOVING_SPHERE) std::memcpy(&prims[k].f[9], &code, 8);
        const auto guard = cs.guard_of_ref.find((int)k);
        if (guard != cs.guard_of_ref.end()) { /* RT_GUARD_FLAG: first guard and count in a sphere's free words */
            const long long first = guard->second.first, count = guard->second.second;
            std::memcpy(&prims[k].f[4], &first, 8), std::memcpy(&prims[k].f[5], &count, 8);
            prims[k].reserved |= RT_GUARD_FLAG;
        }
    }
    return prims;
}

/* references that can tie exactly in t with another one of their instance (see RT_TIE_FLAG); true: some were flagged */
inline bool flag_ties_within_instances(const CompiledScene& cs, std::vector<rtr_node>& prims) {
    bool any_tie = false;
    for (const FInst& I : cs.inst) {
        std::map<std::vector<uint64_t>, std::vector<int>> groups; /* same plane / same sphere */
        auto bits = [](double v) {
            uint64_t u;
            std::memcpy(&u, &v, 8);
            return u;
        };
        for (int r = I.ref_first; r < I.ref_first + I.n_ref; ++r) {
            const rtr_node& n = prims[r];
            if (n.type >= RTR_NODE_XY_RECT)
                groups[{(uint64_t)n.type, bits(n.f[4])}].push_back(r);
            else if (n.type == RTR_NODE_SPHERE)
                groups[{(uint64_t)n.type, bits(n.f[0]), bits(n.f[1]), bits(n.f[2]), bits(std::fabs(n.f[3]))}].push_back(r);
        }
        for (const auto& g : groups) {
            const std::vector<int>& v = g.second;
            if (v.size() > 512) { /* a huge coplanar set (tiled floor): flag all rather than test every pair */
                for (int r : v) prims[r].reserved |= RT_TIE_FLAG;
                any_tie = true;
                continue;
            }
            for (size_t x = 0; x < v.size(); ++x)
                for (size_t y = x + 1; y < v.size(); ++y) {
                    rtr_node &p = prims[v[x]], &q = prims[v[y]];
                    const bool overlap = p.type == RTR_NODE_SPHERE ||
                                         (std::max(p.f[0], q.f[0]) <= std::min(p.f[1], q.f[1]) &&
                                          std::max(p.f[2], q.f[2]) <= std::min(p.f[3], q.f[3]));
                    if (overlap) p.reserved |= RT_TIE_FLAG, q.reserved |= RT_TIE_FLAG, any_tie = true;
                }
        }
    }
    return any_tie;
}

/* Ties ACROSS instances of a sub-scene.  Instances are scanned in the order their first primitive is
 * visited and every test accepts t == t_max, so of two instances the later one wins a tie -- which is the
 * reference's choice (it keeps what it visits later) unless the EARLIER instance holds the later-visited
 * primitive (all primitives under the same transform chain share an instance: [wall, box, floor] puts the
 * floor into the first instance, in front of the box whose bottom face lies in its plane).  Exactly those
 * pairs -- rects whose planes coincide in world space, visiting order against instance order -- get the
 * tie flag; their visiting positions then decide.  A y-plane keeps its orientation under every chain
 * (translate, rotate_y), x- and z-planes under translations only; rotated side faces of different
 * chains are not looked at.  True: some were flagged. */
inline bool flag_ties_across_instances(const CompiledScene& cs, std::vector<rtr_node>& prims) {
    bool any_tie = false;
    for (const FSub& sub : cs.subs) {
        struct PlaneRef {
            double k;
            int axis, inst, ref, visit;
        };
        std::vector<PlaneRef> planes;
        for (int ii = sub.inst_first; ii < sub.inst_first + sub.n_inst; ++ii) {
            const FInst& I = cs.inst[ii];
            double off[3] = {0, 0, 0};
            bool rotated = false;
            for (int k = 0; k < I.n_xf; ++k) {
                const FXf& x = cs.xf[I.xf_first + k];
                if (x.type == RTR_NODE_TRANSLATE)
                    off[0] += x.f[0], off[1] += x.f[1], off[2] += x.f[2];
                else
                    rotated = true;
            }
            for (int r = I.ref_first; r < I.ref_first + I.n_ref; ++r) {
                const rtr_node& n = prims[r];
                if (n.type < RTR_NODE_XY_RECT) continue;
                const int axis = n.type == RTR_NODE_XY_RECT ? 2 : (n.type == RTR_NODE_XZ_RECT ? 1 : 0);
                if (rotated && axis != 1) continue;
                planes.push_back({n.f[4] + off[axis], axis, ii, r, n.reserved & ~RT_TIE_FLAG});
            }
        }
        std::sort(planes.begin(), planes.end(), [](const PlaneRef& a, const PlaneRef& b) {
            return a.axis != b.axis ? a.axis < b.axis : a.k < b.k;
        });
        for (size_t lo = 0; lo < planes.size();) { /* clusters of (nearly) the same world plane */
            size_t hi = lo + 1;
            while (hi < planes.size() && planes[hi].axis == planes[lo].axis &&
                   planes[hi].k - planes[hi - 1].k <= 1e-9 * std::max(1.0, std::fabs(planes[hi].k)))
                ++hi;
            if (hi - lo > 1) {
                std::vector<PlaneRef> cl(planes.begin() + lo, planes.begin() + hi);
                std::sort(cl.begin(), cl.end(), [](const PlaneRef& a, const PlaneRef& b) { return a.inst < b.inst; });
                /* flag P (earlier instance) and Q (later instance) whenever visit(P) > visit(Q) */
                std::vector<int> max_before(cl.size()), min_after(cl.size());
                int mx = -1;
                for (size_t i = 0, j = 0; i < cl.size(); i = j) { /* per instance block */
                    for (j = i; j < cl.size() && cl[j].inst == cl[i].inst; ++j) max_before[j] = mx;
                    for (size_t q = i; q < j; ++q) mx = std::max(mx, cl[q].visit);
                }
                int mn = INT32_MAX;
                for (size_t j = cl.size(), i; j > 0; j = i) {
                    for (i = j; i > 0 && cl[i - 1].inst == cl[j - 1].inst; --i) min_after[i - 1] = mn;
                    for (size_t q = i; q < j; ++q) mn = std::min(mn, cl[q].visit);
                }
                /* (a sub-scene with a top tree meets its instances in any order: every such pair then) */
                const bool any_order = sub.top_root >= 0;
                for (size_t q = 0; q < cl.size(); ++q)
                    if (max_before[q] > cl[q].visit || min_after[q] < cl[q].visit ||
                        (any_order && (max_before[q] >= 0 || min_after[q] < INT32_MAX)))
                        prims[cl[q].ref].reserved |= RT_TIE_FLAG, any_tie = true;
            }
            lo = hi;
        }
    }
    return any_tie;
}

/* FLeaf record of every reference */
inline std::vector<FLeaf> build_leaf_records(const CompiledScene& cs, const std::vector<rtr_node>& prims) {
    std::vector<FLeaf> out(prims.size());
    for (size_t r = 0; r < prims.size(); ++r) {
        FLeaf L{};
        const rtr_node& n = prims[r];
        const int nf = n.type == RTR_NODE_SPHERE ? 4 : (n.type == RTR_NODE_MOVING_SPHERE ? 0 : 5);
        for (int k = 0; k < nf; ++k) L.f[k] = n.f[k];
        L.type = n.type, L.tag = n.reserved;
        out[r] = L;
    }
    return out;
}

/* FInst::scan_first / run[] of every linearly scanned instance; `prims` = the per-reference node records with their tie
 * flags.  Instances whose references do not fit RT_INST_RUNS_MAX runs, or that hold a tie-capable reference (its visiting
 * position takes part in the test), keep the generic loop. */
inline void build_scan_runs(CompiledScene& cs, const std::vector<rtr_node>& prims) {
    cs.scan.clear();
    for (FInst& I : cs.inst) {
        I.flags &= ~RT_INST_RUNS;
        I.scan_first = 0;
        I.runs = 0;
        if (I.bvh_root >= 0 || I.n_ref == 0) continue;
        std::vector<std::pair<int, int>> runs; /* type, count */
        std::vector<double> data;
        bool ok = true;
        const int kBox = RTR_NODE_SPHERE + RT_RUN_BOX;
        auto same = [](double a, double b) { return std::memcmp(&a, &b, 8) == 0; };
        /* the six references from r on are the sides of one box, in box.h's order and with its extents */
        auto box_at = [&](int r) {
            if (r + 6 > I.ref_first + I.n_ref) return false;
            const rtr_node* p = &prims[r];
            static const int want_type[6] = {RTR_NODE_XY_RECT, RTR_NODE_XY_RECT, RTR_NODE_XZ_RECT,
                                             RTR_NODE_XZ_RECT, RTR_NODE_YZ_RECT, RTR_NODE_YZ_RECT};
            for (int k = 0; k < 6; ++k)
                if (p[k].type != want_type[k] || (p[k].reserved & RT_TIE_FLAG)) return false;
            const double x0 = p[0].f[0], x1 = p[0].f[1], y0 = p[0].f[2], y1 = p[0].f[3], z1 = p[0].f[4], z0 = p[1].f[4];
            const double want[6][5] = {{x0, x1, y0, y1, z1}, {x0, x1, y0, y1, z0}, {x0, x1, z0, z1, y1},
                                       {x0, x1, z0, z1, y0}, {y0, y1, z0, z1, x1}, {y0, y1, z0, z1, x0}};
            for (int k = 0; k < 6; ++k)
                for (int c = 0; c < 5; ++c)
                    if (!same(p[k].f[c], want[k][c])) return false;
            return true;
        };
        for (int r = I.ref_first; r < I.ref_first + I.n_ref && ok;) {
            const rtr_node& n = prims[r];
            if (n.reserved & RT_TIE_FLAG) ok = false;
            const bool box = box_at(r);
            /* (a guarded run is read by the kernels of guarded scenes only -- RT_TRAV_FLAT_GUARD --, the others that meet
             * such an instance scan it through the generic loop) */
            const bool guarded = (n.reserved & RT_GUARD_FLAG) != 0;
            const int type = box ? kBox : (guarded ? RTR_NODE_SPHERE + RT_RUN_GUARDED : n.type);
            if (runs.empty() || runs.back().first != type || runs.back().second == RT_RUN_COUNT_MAX) runs.push_back({type, 0});
            ++runs.back().second;
            if (guarded) { /* centre, radius, first guard and guard count (as the integers' bits): six words */
                data.insert(data.end(), n.f, n.f + 6);
                r += 1;
            } else if (box) {
                const double rec[6] = {n.f[0], n.f[1], n.f[2], n.f[3], prims[r + 1].f[4], n.f[4]}; /* x0 x1 y0 y1 z0 z1 */
                data.insert(data.end(), rec, rec + 6);
                r += 6;
            } else {
                const int nf = n.type == RTR_NODE_SPHERE ? 4 : (n.type == RTR_NODE_MOVING_SPHERE ? 9 : 5);
                data.insert(data.end(), n.f, n.f + nf);
                r += 1;
            }
        }
        if (!ok || (int)runs.size() > RT_INST_RUNS_MAX) continue;
        I.scan_first = (int32_t)cs.scan.size();
        for (size_t k = 0; k < runs.size(); ++k)
            I.runs |= (uint64_t)((runs[k].first - RTR_NODE_SPHERE) << RT_RUN_COUNT_BITS | runs[k].second) << (RT_RUN_BITS * k);
        cs.scan.insert(cs.scan.end(), data.begin(), data.end());
        for (size_t k = 0; k < 6; ++k) I.head[k] = k < data.size() ? data[k] : 0.0;
        I.flags |= RT_INST_RUNS;
    }
    cs.scan.resize(cs.scan.size() + 16, 0.0); /* the two-records-per-trip loads never leave the array */
}

/* FMat: materials with their solid textures' values inline */
inline std::vector<FMat> build_materials(const rtr_scene_desc* s) {
    std::vector<FMat> fm((size_t)s->n_materials);
    auto solid = [&](int t) { return t >= 0 && s->textures[t].type == RTR_TEX_SOLID; };
    auto clampd = [](double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }; /* rtweekend.h:40-46 */
    for (int k = 0; k < s->n_materials; ++k) {
        const rtr_material& m = s->materials[k];
        FMat f{};
        f.type = m.type;
        for (int q = 0; q < 4; ++q) f.tex[q] = m.tex[q], f.f[q] = m.f[q];
        switch (m.type) {
        case RTR_MAT_LAMBERTIAN:
        case RTR_MAT_DIFFUSE_LIGHT:
        case RTR_MAT_ISOTROPIC: f.solid = solid(m.tex[0]); break;
        case RTR_MAT_PBR: f.solid = solid(m.tex[0]) && solid(m.tex[1]) && solid(m.tex[2]) && m.tex[3] < 0; break;
        default: f.solid = 1; /* metal, dielectric: no texture */
        }
        if (f.solid && m.type != RTR_MAT_METAL && m.type != RTR_MAT_DIELECTRIC) {
            for (int q = 0; q < 3; ++q) f.albedo[q] = s->textures[m.tex[0]].f[q];
            if (m.type == RTR_MAT_PBR) {
                f.rough = clampd(s->textures[m.tex[1]].f[0], 0.01, 1.0);
                f.metal = s->textures[m.tex[2]].f[0];
            }
        }
        fm[(size_t)k] = f;
    }
    return fm;
}

/* DScene::shared_div -- div_shared's range argument: numerators are differences of scene coordinates and ray origins */
inline bool shared_div_allowed(const rtr_scene_desc* s, const CompiledScene& cs) {
    for (int k = 0; k < s->n_nodes; ++k) {
        const rtr_node& n = s->nodes[k];
        const int nf = n.type == RTR_NODE_TRANSLATE ? 3 : n.type == RTR_NODE_SPHERE ? 4 : n.type == RTR_NODE_MOVING_SPHERE ? 9
                       : n.type >= RTR_NODE_XY_RECT ? 5 : 0;
        for (int q = 0; q < nf; ++q)
            if (!(std::fabs(n.f[q]) <= 0x1p60)) return false;
        /* moving_sphere::center(time) scales (c1 - c0) by (time - t0) / (t1 - t0) */
        if (n.type == RTR_NODE_MOVING_SPHERE && !(std::fabs(n.f[7] - n.f[6]) >= 0x1p-20)) return false;
    }
    if (!(std::fabs(s->camera.time0) <= 0x1p60 && std::fabs(s->camera.time1) <= 0x1p60)) return false;
    for (const FInst& I : cs.inst)
        if (I.n_xf > 30) return false;
    return !getenv("RTR_NO_SHARED_DIV"); /* experiments: the plain divisions */
}

/* FInst::shape of a chain (RT_SHAPE_*): which straight-line block of trace_pair takes a ray pair into the frame */
inline int frame_shape(const FInst& I) {
    if (I.n_xf == 0) return RT_SHAPE_NONE;
    if (I.n_xf > RT_INST_XF_INLINE) return RT_SHAPE_OTHER;
    int code = 0; /* two bits per op, outermost first: 1 translate, 2 rotate_y */
    for (int k = 0; k < I.n_xf; ++k) {
        if (I.xf_type[k] == RTR_NODE_TRANSLATE) {
            code = code << 2 | 1;
        } else if (I.xf_type[k] == RTR_NODE_ROTATE_Y) {
            code = code << 2 | 2;
        } else {
            return RT_SHAPE_OTHER;
        }
    }
    switch (code) {
    case 1: return RT_SHAPE_T;
    case 2: return RT_SHAPE_R;
    case 1 << 2 | 2: return RT_SHAPE_TR;
    case 2 << 2 | 1: return RT_SHAPE_RT;
    default: return RT_SHAPE_OTHER; /* T T, R R: rare enough to keep the generic loop */
    }
}

/* trace_pair's scenes (DScene::pair_cast): flat, lit (without lights no shadow ray is ever cast, and the pair walk
 * would test a dummy ray against every record: scene 7, 7 515 -> 6 122 Msamples/s), few enough instances that no
 * instance box is tested, every instance a packed scan without moving spheres, shared divisions allowed; the others
 * keep the split casts.  `cs` with its scan runs, `d` with n_finst, top_root0 and shared_div. */
inline bool pair_cast_allowed(const rtr_scene_desc* s, const CompiledScene& cs, const DScene& d, bool flat_scene) {
    if (!(flat_scene && s->n_lights > 0 && d.shared_div && d.top_root0 < 0 && d.n_finst > 0 && d.n_finst <= RT_FAST_NO_BOX_MAX))
        return false;
    for (int k = 0; k < d.n_finst; ++k) {
        const FInst& I = cs.inst[k];
        if (!(I.flags & RT_INST_RUNS)) return false;
        if (!(I.flags & RT_INST_KEEP_Y)) return false; /* trace_pair reads every frame's d.y from the world ray */
        for (uint64_t runs = I.runs; runs != 0; runs >>= RT_RUN_BITS) {
            const int type = RTR_NODE_SPHERE + (int)((runs >> RT_RUN_COUNT_BITS) & 7);
            if (type != RTR_NODE_SPHERE && type != RTR_NODE_XY_RECT && type != RTR_NODE_XZ_RECT && type != RTR_NODE_YZ_RECT &&
                type != RTR_NODE_SPHERE + RT_RUN_BOX)
                return false;
        }
    }
    return true;
}

/* FFin of every reference of a flat scene, or nothing where some reference does not fit the record: an instance of
 * sub-scene 0 with more than RT_INST_XF_INLINE transform ops, a moving sphere, an RT_EXIT_LONG code.  The two-bit wrapper
 * code of build_prims is reduced to "levels, then one flip bit" (see FFin::flip). */
inline std::vector<FFin> build_finish(const CompiledScene& cs, const std::vector<rtr_node>& prims, bool flat) {
    std::vector<FFin> out;
    if (!flat || !cs.ok || cs.subs.empty()) return out;
    const FSub& sub0 = cs.subs[0];
    out.assign(prims.size(), FFin{});
    for (int ii = sub0.inst_first; ii < sub0.inst_first + sub0.n_inst; ++ii) {
        const FInst& I = cs.inst[ii];
        if (I.n_xf > RT_INST_XF_INLINE) return {};
        for (int r = I.ref_first; r < I.ref_first + I.n_ref; ++r) {
            const rtr_node& n = prims[r];
            unsigned long long code;
            std::memcpy(&code, &n.f[9], 8);
            if (n.type == RTR_NODE_MOVING_SPHERE || code == RT_EXIT_LONG) return {};
            FFin F{};
            F.kind = n.type == RTR_NODE_SPHERE ? RT_FIN_SPHERE : (n.type == RTR_NODE_YZ_RECT ? 0 : (n.type == RTR_NODE_XZ_RECT ? 1 : 2));
            F.mat = n.a;
            F.levels = I.n_xf;
            for (int k = 0; k < I.n_xf; ++k) {
                if (I.xf_type[k] == RTR_NODE_ROTATE_Y) F.levels |= k == 0 ? RT_FIN_ROT0 : RT_FIN_ROT1;
                for (int q = 0; q < 3; ++q) F.op[k][q] = I.xf_f[k][q];
            }
            int left = I.n_xf, flips = 0; /* levels not yet left, flip_face wrappers since the last one */
            for (; code != 0; code >>= 2) {
                if ((code & 3) == 2)
                    ++flips;
                else
                    --left, flips = 0;
            }
            if (left != 0) return {}; /* (the code names every level of the chain once) */
            F.flip = flips & 1;
            for (int q = 0; q < 4; ++q) F.g[q] = n.f[q];
            out[(size_t)r] = F;
        }
    }
    return out;
}

/* the material and light class: lean_materials, quad_lights_only, n_material_types, n_materials */
inline void material_facts(const rtr_scene_desc* s, SceneFacts& f) {
    f.n_materials = s->n_materials;
    f.lean_materials = true;
    unsigned type_mask = 0;
    for (int k = 0; k < s->n_materials; ++k) type_mask |= 1u << s->materials[k].type;
    f.n_material_types = __builtin_popcount(type_mask);
    f.quad_lights_only = true;
    for (int k = 0; k < s->n_lights; ++k)
        if (s->lights[k].type != RTR_LIGHT_QUAD) f.quad_lights_only = false;
    if (!f.quad_lights_only) f.lean_materials = false; /* the lean kernels know QuadLights only */
    for (int k = 0; k < s->n_materials; ++k) {
        const rtr_material& m = s->materials[k];
        if (m.type != RTR_MAT_LAMBERTIAN && m.type != RTR_MAT_DIFFUSE_LIGHT) f.lean_materials = false;
        else if (s->textures[m.tex[0]].type != RTR_TEX_SOLID) f.lean_materials = false;
    }
}

/* SceneFacts::uv_order_dependent: some moving_sphere carries a material that reads (u,v) */
inline bool uv_order_dependent(const rtr_scene_desc* s, const rtr_scene_info& info) {
    if (!info.needs_uv) return false;
    std::function<bool(int, int)> tex_reads_uv = [&](int t, int guard) {
        if (t < 0 || guard > 8) return false;
        const rtr_texture& x = s->textures[t];
        if (x.type == RTR_TEX_IMAGE) return x.a >= 0;
        if (x.type == RTR_TEX_CHECKER) return tex_reads_uv(x.a, guard + 1) || tex_reads_uv(x.b, guard + 1);
        return false;
    };
    for (int k = 0; k < s->n_nodes; ++k) {
        if (s->nodes[k].type != RTR_NODE_MOVING_SPHERE) continue;
        const rtr_material& m = s->materials[s->nodes[k].a];
        const int n_tex = m.type == RTR_MAT_PBR ? 4 : (m.type == RTR_MAT_METAL || m.type == RTR_MAT_DIELECTRIC ? 0 : 1);
        for (int q = 0; q < n_tex; ++q)
            if (tex_reads_uv(m.tex[q], 0)) return true;
    }
    return false;
}

} // namespace rtc

/* `s` has passed validation and `info` holds what the validator found; the fast_* members, program_steps and top_trees
 * are filled here.  RTR_TOP_MIN and RTR_NO_SHARED_DIV are read at every call.  The order matters: tie flags before leaf
 * records and scan runs (both read them), scan runs before inst[] is final, pair_cast after the runs exist. */
inline LoweredScene lower_scene(const rtr_scene_desc* s, rtr_scene_info& info) {
    LoweredScene L;
    CompiledScene& cs = L.cs = rtc::compile_validated(s, info);
    SceneFacts& f = L.facts;
    L.steps = rtc::build_steps(cs);
    L.visits = rtc::build_visits(cs, L.steps);
    f.machine_ok = !L.visits.empty();
    for (const FStep& st : L.steps) f.guarded_program |= st.kind == 3 || st.n_xf > 0 || st.n_exit > 0;
    L.prims = rtc::build_prims(s, cs);
    bool any_tie = rtc::flag_ties_within_instances(cs, L.prims);
    any_tie |= rtc::flag_ties_across_instances(cs, L.prims);
    L.leaves = rtc::build_leaf_records(cs, L.prims);
    rtc::build_scan_runs(cs, L.prims);
    for (FInst& I : cs.inst) I.shape = rtc::frame_shape(I);
    f.fast_stack_words = cs.stack_words;
    /* (guarded references -- hollow spheres -- are tested by the generic loop of the kernels that know about ties: the
     * flat kernels carry neither) */
    f.flat_scene = cs.ok && cs.bvh.empty() && !any_tie && cs.guard_of_ref.empty();
    f.flat_guarded = cs.ok && cs.bvh.empty() && !any_tie && !cs.guard_of_ref.empty(); /* the megakernel's RT_TRAV_FLAT_GUARD */
    f.walk_extra_words = cs.n_compiled_subtrees ? cs.stack_words : 0;
    DScene& d = L.ds;
    std::memset(&d, 0, sizeof d); /* padding bytes included: the record goes to the device whole */
    d.n_finst = cs.ok ? cs.subs[0].n_inst : 0;
    d.top_root0 = cs.ok ? cs.subs[0].top_root : -1;
    d.world_inst0 = cs.ok ? cs.subs[0].world_inst : -1;
    d.world_linear0 = cs.ok ? cs.subs[0].world_linear : 0;
    d.top_bound0 = cs.ok ? cs.subs[0].top_bound : 0.0f;
    d.n_fstep = (int32_t)L.steps.size();
    d.fstep_tail = cs.step_tail;
    d.n_fvisit = (int32_t)L.visits.size();
    d.camera = s->camera;
    for (int k = 0; k < 3; ++k) d.background[k] = s->background[k];
    d.root = s->root;
    d.n_nodes = s->n_nodes;
    d.n_lights = s->n_lights;
    d.needs_uv = info.needs_uv;
    d.shared_div = rtc::shared_div_allowed(s, cs);
    d.pair_cast = rtc::pair_cast_allowed(s, cs, d, f.flat_scene);
    f.top_tree = d.top_root0 >= 0, f.needs_uv = info.needs_uv != 0, f.pair_cast = d.pair_cast != 0;
    L.finish = rtc::build_finish(cs, L.prims, f.flat_scene || f.flat_guarded);
    rtc::material_facts(s, f);
    f.uv_order_dependent = rtc::uv_order_dependent(s, info);
    L.mats = rtc::build_materials(s);
    f.t_lo = std::min(0.0, std::min(s->camera.time0, s->camera.time1)); /* Builder::run of rt_compile.h */
    f.t_hi = std::max(0.0, std::max(s->camera.time0, s->camera.time1));
    f.camera_times_small = std::fabs(s->camera.time0) <= 0x1p60 && std::fabs(s->camera.time1) <= 0x1p60;
    return L;
}
