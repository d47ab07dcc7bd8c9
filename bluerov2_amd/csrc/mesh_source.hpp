// mesh_source.hpp -- the host side of the range stage's triangle mesh (mesh_kernel.hip: mesh_eval_kernel, inspect_mesh_tick_kernel; the public
// names are brov_mesh_* of include/bluerov2_nmpc_mesh.h): the argument checks, the build (mesh_bvh.hpp), the structure on the device and its
// summary.  A member of InspectSource (inspect_source.hpp), which launches the mesh kernels iff `set()`.  The mesh can be replaced and
// removed, so its two blocks are the stage's own and not the owner's: they are freed when the mesh goes and when the owner does.  Host code
// only, header only.
#pragma once
#include <cmath>
#include <string>

#include "host_common.hpp"
#include "mesh_device.hpp"

namespace brov {

struct MeshSource {
    MeshDev dev;
    brov_mesh_summary info{};
    void* blocks[2] = {nullptr, nullptr};

    bool set() const { return dev.n_tris > 0; }
    void release() {
        for (void*& p : blocks)
            if (p) { (void)hipFree(p); p = nullptr; }
        dev = MeshDev{};
        info = brov_mesh_summary{};
    }
    void destroy() { release(); }

    int set_host(int64_t n, const double* tri, int32_t leaf, const CallCtx& c) {
        if (n < 0 || n > BROV_MESH_MAX_TRIANGLES) return c.refuse("the mesh holds 0 ... BROV_MESH_MAX_TRIANGLES triangles");
        if (leaf < 0 || leaf > BROV_MESH_MAX_LEAF) return c.refuse("leaf must lie in 0 ... BROV_MESH_MAX_LEAF (0: the default)");
        if (n > 0 && !tri) return c.refuse("null argument");
        for (int64_t j = 0; j < n * 9; j++)
            if (!std::isfinite(tri[j])) return c.refuse("a coordinate is not finite");
        if (int rc = c.wait()) return rc;
        if (n == 0) { release(); return BROV_OK; }
        MeshBvh h;
        mesh_bvh_build(n, tri, leaf ? leaf : BROV_MESH_DEFAULT_LEAF, h);
        const size_t nb = h.nodes.size() * sizeof(MeshNode), tb = h.tris.size() * sizeof(MeshTri);
        ScopedDeviceBuffer<char> nd, td;
        if (nd.init(nb) != hipSuccess || td.init(tb) != hipSuccess) {
            (void)hipGetLastError();
            c.err = std::string(c.who) + ": hipMalloc of " + std::to_string(nb + tb) + " bytes for the mesh failed";
            return BROV_ERR_ALLOC;
        }
        BROV_HIPCHK(c.err, hipMemcpy(nd.p, h.nodes.data(), nb, hipMemcpyHostToDevice));
        BROV_HIPCHK(c.err, hipMemcpy(td.p, h.tris.data(), tb, hipMemcpyHostToDevice));
        release();
        blocks[0] = nd.release(); blocks[1] = td.release();
        dev.nodes = (const MeshNode*)blocks[0]; dev.tris = (const MeshTri*)blocks[1];
        dev.n_nodes = (int32_t)h.nodes.size(); dev.n_tris = (int32_t)h.tris.size();
        info.triangles = n; info.nodes = (int64_t)h.nodes.size(); info.leaves = h.leaves; info.device_bytes = (int64_t)(nb + tb);
        info.pad = h.pad; info.depth = h.depth; info.leaf = h.leaf;
        return BROV_OK;
    }
    int get_info(brov_mesh_summary* out, const CallCtx& c) const {
        if (!out) return c.refuse("null argument");
        *out = info;
        return BROV_OK;
    }
};

}  // namespace brov
