// mesh_refusals_main.cpp -- the argument checks of the range stage's mesh (bluerov2_amd/csrc/mesh_source.hpp, a member of
// inspect_source.hpp's InspectSource) run without a device, for tests/test_mesh_abi.py: every refusal of brov_mesh_set_host, of
// brov_mesh_eval_host without a mesh and of a step with neither box nor mesh, with its code and text, and the proof that none of them waited
// for or allocated anything.  Prints "<case> => <code> <text>" per case.  Host code only; the launchers the headers name are stubs that
// abort: no refused call may reach them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "bluerov2_nmpc.h"
#include "inspect_source.hpp"

namespace brov {
void launch_range_eval(const brov_range_params&, const RangeScene&, const double*, int, long long, const double*, double*, int32_t*, double*, double*,
                       hipStream_t) { std::abort(); }
void launch_inspect_eval(const brov_inspect_params&, int, const brov_inspect_state*, const double*, const double*, const double*, brov_inspect_state*,
                         brov_result*, brov_inspect_stats*, hipStream_t) { std::abort(); }
void launch_inspect_tick(const brov_range_params&, const RangeScene&, const double*, const brov_inspect_params&, const InspectDev&, int, long long,
                         const double*, const double*, brov_result*, hipStream_t) { std::abort(); }
void launch_mesh_eval(const brov_range_params&, const RangeScene&, const MeshDev&, const double*, int, long long, const double*, double*, int32_t*, double*,
                      double*, long long*, hipStream_t) { std::abort(); }
void launch_inspect_mesh_tick(const brov_range_params&, const RangeScene&, const MeshDev&, const double*, const brov_inspect_params&, const InspectDev&, int,
                              long long, const double*, const double*, brov_result*, hipStream_t) { std::abort(); }
}  // namespace brov

int main() {
    using namespace brov;
    const size_t B = 3;
    int waits = 0;
    DeviceAllocs mem;
    std::string err;
    const CallCtx ctx{[&waits] { waits++; return BROV_OK; }, mem, err, "brov_mesh_test"};
    InspectSource in;
    in.B = B;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto report = [&](const char* name, int rc) { std::printf("%s => %d %s\n", name, rc, err.c_str()); err.clear(); };

    std::vector<double> tri(4 * 9);
    for (size_t j = 0; j < tri.size(); j++) tri[j] = 0.25 * (double)((j * 7) % 11);
    report("n = -1", in.mesh.set_host(-1, tri.data(), 0, ctx));
    report("n = 2^20 + 1", in.mesh.set_host((1LL << 20) + 1, tri.data(), 0, ctx));   // refused before a coordinate is read
    report("null triangles", in.mesh.set_host(4, nullptr, 0, ctx));
    report("leaf -1", in.mesh.set_host(4, tri.data(), -1, ctx));
    report("leaf 9", in.mesh.set_host(4, tri.data(), 9, ctx));
    tri[13] = nan; report("NaN", in.mesh.set_host(4, tri.data(), 4, ctx));
    tri[13] = -inf; report("-inf", in.mesh.set_host(4, tri.data(), 4, ctx));
    tri[13] = 1.0; tri[35] = inf; report("inf in the last", in.mesh.set_host(4, tri.data(), 8, ctx));

    // the eval call that needs a mesh, and a step
    double x[12 * B] = {}, range[B];
    int32_t hits[B];
    int64_t visits[2 * B];
    report("eval without a mesh", in.range_eval_host(0, x, range, hits, nullptr, nullptr, nullptr, ctx, visits, true));
    report("eval null", in.range_eval_host(0, nullptr, range, hits, nullptr, nullptr, nullptr, ctx, visits, true));
    in.on = true;
    report("neither box nor mesh", in.steps_ok(0, 1, 0, ctx));
    in.mesh.dev.n_tris = 1;   // (what a mesh in force looks like to the checks)
    if (in.steps_ok(0, 1, 0, ctx) != BROV_OK) return 2;
    report("mesh and comp > 0", in.steps_ok(0, 1, 1, ctx));
    in.mesh.dev.n_tris = 0;
    brov_mesh_summary info;
    report("null info", in.mesh.get_info(nullptr, ctx));
    if (in.mesh.get_info(&info, ctx) != BROV_OK || info.triangles != 0 || info.nodes != 0 || info.leaf != 0) return 3;
    std::printf("waits => %d\nallocations => %d\n", waits, (int)(in.sigma != nullptr || in.dev.state != nullptr || in.mesh.blocks[0] != nullptr || !mem.ptrs.empty()));
    return 0;
}
