/*
 * rt_validate.h -- the scene validator of rtr_validate_scene / rtr_upload_scene: every index, count and parameter of an
 * rtr_scene_desc checked, and the traversal stack the graph needs measured, before anything is lowered or uploaded.
 * Host only, no HIP call; rt_device.h gives the stack-frame sizes the device walk uses.
 */
#pragma once

#include "rt_device.h"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

/* scene validation + traversal stack analysis */
struct Validator {
    const rtr_scene_desc* s;
    std::string msg;
    std::vector<int> state;  /* 0 new, 1 on DFS stack, 2 done */
    std::vector<int> need;   /* stack words used below a node (see traverse()) */
    std::vector<int> depth;
    std::vector<char> media; /* subtree contains a constant_medium */
    int code = RTR_OK;

    bool bad(int c, const std::string& m) {
        if (code == RTR_OK) {
            code = c;
            msg = m;
        }
        return false;
    }
    bool node_ix(int i) const { return i >= 0 && i < s->n_nodes; }

    bool texture_ok(int ix, int guard) {
        if (ix < 0 || ix >= s->n_textures) return bad(RTR_ERR_INVALID, "texture index out of range");
        if (guard > 7) return bad(RTR_ERR_UNSUPPORTED, "checker textures nested deeper than 8");
        const rtr_texture& t = s->textures[ix];
        switch (t.type) {
        case RTR_TEX_SOLID: return true;
        case RTR_TEX_CHECKER: return texture_ok(t.a, guard + 1) && texture_ok(t.b, guard + 1);
        case RTR_TEX_NOISE:
            if (t.a < 0 || t.a >= s->n_perlin) return bad(RTR_ERR_INVALID, "perlin table index out of range");
            return true;
        case RTR_TEX_IMAGE:
            if (t.a >= s->n_images) return bad(RTR_ERR_INVALID, "image index out of range");
            if (t.a >= 0) {
                const rtr_image& im = s->images[t.a];
                /* width * height * 3 of two positive int32 fits a uint64; the offset is compared first so
                 * the sum cannot wrap */
                if (im.width <= 0 || im.height <= 0 || im.offset > s->n_image_bytes ||
                    (uint64_t)im.width * (uint64_t)im.height * 3 > s->n_image_bytes - im.offset)
                    return bad(RTR_ERR_INVALID, "image texels out of range");
            }
            return true;
        default: return bad(RTR_ERR_UNSUPPORTED, "unknown texture type");
        }
    }

    bool material_ok(int ix) {
        if (ix < 0 || ix >= s->n_materials) return bad(RTR_ERR_INVALID, "material index out of range");
        const rtr_material& m = s->materials[ix];
        switch (m.type) {
        case RTR_MAT_LAMBERTIAN:
        case RTR_MAT_DIFFUSE_LIGHT:
        case RTR_MAT_ISOTROPIC: return texture_ok(m.tex[0], 0);
        case RTR_MAT_METAL:
        case RTR_MAT_DIELECTRIC: return true;
        case RTR_MAT_PBR:
            if (!texture_ok(m.tex[0], 0) || !texture_ok(m.tex[1], 0) || !texture_ok(m.tex[2], 0)) return false;
            return m.tex[3] < 0 || texture_ok(m.tex[3], 0);
        default: return bad(RTR_ERR_UNSUPPORTED, "unknown material type");
        }
    }

    /* children of a node by position (no per-visit copies: a hittable_list can hold a million of them) */
    int child_count(const rtr_node& n) const {
        switch (n.type) {
        case RTR_NODE_BVH: return 2;
        case RTR_NODE_LIST: return n.b;
        case RTR_NODE_TRANSLATE:
        case RTR_NODE_ROTATE_Y:
        case RTR_NODE_FLIP_FACE:
        case RTR_NODE_MEDIUM: return 1;
        default: return 0;
        }
    }
    int child_at(const rtr_node& n, int k) const {
        if (n.type == RTR_NODE_BVH) return k == 0 ? n.a : n.b;
        if (n.type == RTR_NODE_LIST) return s->list_children[n.a + k];
        return n.a;
    }

    /* iterative post-order DFS over the hittable DAG */
    bool walk(int root) {
        struct Frame {
            int node, next;
        };
        std::vector<Frame> stk;
        stk.push_back({root, 0});
        state[root] = 1;
        while (!stk.empty()) {
            Frame& f = stk.back();
            const rtr_node& n = s->nodes[f.node];
            if (f.next == 0) { /* first visit: check the record itself */
                int n_geom = 0; /* leading f[] entries the scene compiler builds boxes from: must be finite */
                switch (n.type) {
                case RTR_NODE_BVH: /* its box is only ever compared with a ray: any value is safe */
                case RTR_NODE_FLIP_FACE: break;
                case RTR_NODE_TRANSLATE: n_geom = 3; break;
                case RTR_NODE_ROTATE_Y: n_geom = 2; break;
                case RTR_NODE_LIST:
                    if (n.a < 0 || n.b < 0 || (int64_t)n.a + n.b > s->n_list_children)
                        return bad(RTR_ERR_INVALID, "hittable_list children out of range");
                    break;
                case RTR_NODE_MEDIUM:
                    if (!material_ok(n.b)) return false;
                    break;
                case RTR_NODE_SPHERE: n_geom = 4; break;
                case RTR_NODE_MOVING_SPHERE: n_geom = 9; break;
                case RTR_NODE_XY_RECT:
                case RTR_NODE_XZ_RECT:
                case RTR_NODE_YZ_RECT: n_geom = 5; break;
                default: return bad(RTR_ERR_UNSUPPORTED, "unknown hittable node type");
                }
                if (n.type >= RTR_NODE_SPHERE && !material_ok(n.a)) return false;
                for (int k = 0; k < n_geom; ++k)
                    if (!std::isfinite(n.f[k])) return bad(RTR_ERR_INVALID, "non-finite primitive or transform parameter");
            }
            const int m = child_count(n);
            if (f.next < m) {
                int k = child_at(n, f.next++);
                if (!node_ix(k)) return bad(RTR_ERR_INVALID, "hittable child index out of range");
                if (state[k] == 1) return bad(RTR_ERR_INVALID, "hittable graph has a cycle");
                if (state[k] == 0) {
                    state[k] = 1;
                    stk.push_back({k, 0});
                }
                continue;
            }
            /* children done: stack words, depth, media */
            const int me = f.node;
            int u = 0, d = 0;
            char md = 0;
            for (int k = 0; k < m; ++k) {
                const int ck = child_at(n, k);
                d = std::max(d, depth[ck]);
                md |= media[ck];
            }
            switch (n.type) {
            case RTR_NODE_BVH: u = std::max(2, std::max(1 + need[n.a], need[n.b])); break;
            case RTR_NODE_LIST:
                if (m > RT_LIST_BULK) { /* continuation (2 words) + the child being walked */
                    u = 3;
                    for (int k = 0; k < m; ++k) u = std::max(u, 2 + need[child_at(n, k)]);
                } else {
                    u = m;
                    for (int k = 0; k < m; ++k) u = std::max(u, (m - 1 - k) + need[child_at(n, k)]);
                }
                break;
            case RTR_NODE_TRANSLATE: u = RT_FRAME_TRANSLATE + std::max(1, need[n.a]); break;
            case RTR_NODE_ROTATE_Y: u = RT_FRAME_ROTATE + std::max(1, need[n.a]); break;
            case RTR_NODE_FLIP_FACE: u = RT_FRAME_FLIP + std::max(1, need[n.a]); break;
            case RTR_NODE_MEDIUM:
                if (md) return bad(RTR_ERR_UNSUPPORTED, "constant_medium nested inside a medium boundary");
                u = std::max(1, need[n.a]);
                md = 1;
                break;
            default: break;
            }
            need[me] = u;
            depth[me] = d + 1;
            media[me] = md;
            state[me] = 2;
            stk.pop_back();
        }
        return true;
    }

    int run(rtr_scene_info* info) {
        if (!s) return (bad(RTR_ERR_INVALID, "null scene"), code);
        if (s->abi_version != RTR_ABI_VERSION) return (bad(RTR_ERR_INVALID, "ABI version mismatch"), code);
        if (s->n_nodes >= RT_LIST_MARK) return (bad(RTR_ERR_INVALID, "more than 2^30 nodes"), code);
    if (s->n_nodes <= 0 || s->n_list_children < 0 || s->n_materials < 0 || s->n_textures < 0 ||
            s->n_perlin < 0 || s->n_images < 0 || s->n_lights < 0)
            return (bad(RTR_ERR_INVALID, "negative or empty counts"), code);
        if (!node_ix(s->root)) return (bad(RTR_ERR_INVALID, "root out of range"), code);
        if (!s->nodes || (s->n_list_children && !s->list_children) || (s->n_materials && !s->materials) ||
            (s->n_textures && !s->textures) || (s->n_perlin && !s->perlin) || (s->n_images && !s->images) ||
            (s->n_image_bytes && !s->image_bytes) || (s->n_lights && !s->lights))
            return (bad(RTR_ERR_INVALID, "null array with non-zero count"), code);
        for (int k = 0; k < s->n_lights; ++k) {
            const rtr_light& l = s->lights[k];
            if (l.type < 0 || l.type >= RTR_LIGHT_TYPE_COUNT)
                return (bad(RTR_ERR_UNSUPPORTED, "unknown light type (QuadLight, PointLight, SpotLight, DirectionalLight, EnvironmentLight are on the device)"), code);
            if (l.type == RTR_LIGHT_ENV_MAP) { /* texels and sampling tables live in image_bytes */
                const double w = l.f[0], h = l.f[1], to = l.f[3], tb = l.f[4];
                if (!(w >= 1 && h >= 1 && w <= 65536 && h <= 65536) || w != (double)(int)w || h != (double)(int)h)
                    return (bad(RTR_ERR_INVALID, "environment map size out of range"), code);
                const double nb = (double)s->n_image_bytes;
                const double texel_bytes = w * h * 3 * 4, table_bytes = (h * (2 * w + 2) + (2 * h + 2)) * 8;
                if (!(to >= 0 && tb >= 0) || to != (double)(uint64_t)to || tb != (double)(uint64_t)tb ||
                    (uint64_t)to % 4 || (uint64_t)tb % 8 || to + texel_bytes > nb || tb + table_bytes > nb)
                    return (bad(RTR_ERR_INVALID, "environment map texels / tables out of range or misaligned"), code);
            }
        }
        /* every record is checked, also those the graph under `root` does not reach: upload and the
         * scene-wide facts (material classes, texture classes) loop over whole arrays */
        for (int k = 0; k < s->n_textures; ++k)
            if (!texture_ok(k, 0)) return code;
        for (int k = 0; k < s->n_materials; ++k)
            if (!material_ok(k)) return code;
        /* materials/perlin.h:35 indexes ranvec[perm_x ^ perm_y ^ perm_z]: the device does the same, unchecked */
        for (int k = 0; k < s->n_perlin; ++k)
            for (int i = 0; i < 256; ++i)
                if ((unsigned)s->perlin[k].perm_x[i] > 255u || (unsigned)s->perlin[k].perm_y[i] > 255u ||
                    (unsigned)s->perlin[k].perm_z[i] > 255u)
                    return (bad(RTR_ERR_INVALID, "perlin permutation entry out of range"), code);
        for (int k = 0; k < s->n_nodes; ++k) {
            const rtr_node& n = s->nodes[k];
            if (n.type < 0 || n.type >= RTR_NODE_TYPE_COUNT)
                return (bad(RTR_ERR_UNSUPPORTED, "unknown hittable node type"), code);
            if (n.type >= RTR_NODE_SPHERE && (n.a < 0 || n.a >= s->n_materials))
                return (bad(RTR_ERR_INVALID, "material index out of range"), code);
            if (n.type == RTR_NODE_MEDIUM && (n.b < 0 || n.b >= s->n_materials))
                return (bad(RTR_ERR_INVALID, "material index out of range"), code);
        }
        state.assign(s->n_nodes, 0);
        need.assign(s->n_nodes, 0);
        depth.assign(s->n_nodes, 0);
        media.assign(s->n_nodes, 0);
        if (!walk(s->root)) return code;
        if (info) {
            info->stack_words = std::max(1, need[s->root]);
            info->has_media = media[s->root];
            int inverted = 0;
            for (int k = 0; k < s->n_nodes; ++k)
                if (state[k] == 2 && ((s->nodes[k].type == RTR_NODE_SPHERE && s->nodes[k].f[3] < 0) ||
                                      (s->nodes[k].type == RTR_NODE_MOVING_SPHERE && s->nodes[k].f[8] < 0)))
                    ++inverted;
            info->inverted_boxes = inverted;
            info->graph_depth = depth[s->root];
            int uv = 0;
            for (int k = 0; k < s->n_textures; ++k)
                if (s->textures[k].type == RTR_TEX_IMAGE && s->textures[k].a >= 0) uv = 1;
            info->needs_uv = uv;
        }
        return RTR_OK;
    }
};
