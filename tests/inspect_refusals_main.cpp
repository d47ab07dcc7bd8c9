// inspect_refusals_main.cpp -- the argument checks of the range stage's and the inspection controller's host side
// (bluerov2_amd/csrc/inspect_source.hpp) run without a device, for tests/test_inspect_abi.py: every refusal of brov_range_set_scene_host,
// brov_range_set_host and brov_inspect_set_host, of a step without a scene, with the controller off, behind a predicting delay stage or past
// index 2^24, and of a plant step with another dt, with its code and text, and the proof that none of them waited for or allocated anything.
// Prints "<case> => <code> <text>" per case.  Host code only; the three launchers the header names are stubs that abort: no refused call may
// reach them.
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
}  // namespace brov

int main() {
    using namespace brov;
    const size_t B = 3;
    int waits = 0;
    DeviceAllocs mem;
    std::string err;
    const CallCtx ctx{[&waits] { waits++; return BROV_OK; }, mem, err, "brov_inspect_test"};
    InspectSource in;
    in.B = B;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    auto report = [&](const char* name, int rc) { std::printf("%s => %d %s\n", name, rc, err.c_str()); err.clear(); };

    // the scene
    std::vector<double> lo(9 * 3, 0.0), hi(9 * 3, 1.0);
    report("9 boxes", in.set_scene_host(9, lo.data(), hi.data(), ctx));
    report("-1 boxes", in.set_scene_host(-1, lo.data(), hi.data(), ctx));
    lo[4] = 2.0; report("lo > hi", in.set_scene_host(2, lo.data(), hi.data(), ctx));
    lo[4] = nan; report("lo NaN", in.set_scene_host(2, lo.data(), hi.data(), ctx));
    lo[4] = 0.0; hi[2] = inf; report("hi inf", in.set_scene_host(1, lo.data(), hi.data(), ctx));
    report("null boxes", in.set_scene_host(1, nullptr, nullptr, ctx));

    // the camera
    const brov_range_params good = InspectSource::default_range();
    auto cam = [&](const char* name, brov_range_params p, double sigma1) {
        std::vector<double> sigma(B, 0.01);
        sigma[1] = sigma1;
        report(name, in.set_range_host(&p, sigma.data(), ctx));
    };
    brov_range_params p = good;
    p.roi = 41; cam("roi odd", p, 0.01);
    p.roi = 0; cam("roi 0", p, 0.01);
    p.roi = 66; cam("roi 66", p, 0.01);
    p = good; p.f = 0.0; cam("f = 0", p, 0.01);
    p.f = -1.0; cam("f < 0", p, 0.01);
    p.f = nan; cam("f NaN", p, 0.01);
    p = good; p.cx = inf; cam("cx inf", p, 0.01);
    p = good; p.mount[2] = nan; cam("mount NaN", p, 0.01);
    p = good; p.near = 100.0; cam("near = far", p, 0.01);
    p = good; p.far = 0.05; cam("near > far", p, 0.01);
    cam("sigma < 0", good, -1e-9);
    cam("sigma NaN", good, nan);
    report("null camera", in.set_range_host(nullptr, nullptr, ctx));

    // the controller
    const brov_inspect_params cgood = InspectSource::default_inspect();
    brov_inspect_params c = cgood;
    c.dt = 0.0; report("dt = 0", in.set_host(&c, ctx));
    c.dt = nan; report("dt NaN", in.set_host(&c, ctx));
    c = cgood; c.gains[7] = inf; report("gain inf", in.set_host(&c, ctx));
    c = cgood; c.z_goal = nan; report("z_goal NaN", in.set_host(&c, ctx));
    c = cgood; c.flags = 4; report("flag 4", in.set_host(&c, ctx));
    report("null controller", in.set_host(nullptr, ctx));

    // a step
    report("controller off", in.steps_ok(0, 1, 0, ctx));
    in.on = true;
    report("no box", in.steps_ok(0, 1, 0, ctx));
    in.scene.n = 1;
    report("comp > 0", in.steps_ok(0, 1, 1, ctx));
    report("index 2^24", in.steps_ok((1LL << 24) - 2, 3, 0, ctx));
    report("dt != dt", in.dt_ok(0.05, ctx) == BROV_OK ? in.dt_ok(0.05000000000000001, ctx) : 99);
    if (in.steps_ok((1LL << 24) - 2, 2, 0, ctx) != BROV_OK) return 2;
    in.on = false;
    if (in.dt_ok(0.04, ctx) != BROV_OK) return 3;
    std::printf("waits => %d\nallocations => %d\n", waits, (int)(in.sigma != nullptr || in.dev.state != nullptr));
    return 0;
}
