// imu_refusals_main.cpp -- the argument checks of the IMU/GPS stage's host side (bluerov2_amd/csrc/imu_source.hpp) run without a device, for
// tests/test_imu_abi.py: every refusal of brov_imu_set_host, of a plant step with dt != h and of an index past 2^24, with its code and text, and
// the proof that none of them waited for or allocated anything.  Prints "<case> => <code> <text>" per case.  Host code only; the two launchers
// the header names are stubs that abort: no refused call may reach them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "bluerov2_nmpc.h"
#include "imu_source.hpp"

namespace brov {
void launch_imu_measure(const ImuPar&, const ImuDev&, const ImuOut&, int, long long, bool, const double*, hipStream_t) { std::abort(); }
void launch_imu_eval(const ImuPar&, const ImuDev&, const ImuOut&, int, long long, const double*, const double*, const double*, const int32_t*,
                     hipStream_t) { std::abort(); }
}  // namespace brov

int main() {
    using namespace brov;
    const size_t B = 3;
    int waits = 0;
    DeviceAllocs mem;
    std::string err;
    const CallCtx ctx{[&waits] { waits++; return BROV_OK; }, mem, err, "brov_imu_test"};
    ImuSource im;
    im.B = B;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const brov_imu_params good{0.01, 9.81, 2, 0, 7};
    auto report = [&](const char* name, int rc) { std::printf("%s => %d %s\n", name, rc, err.c_str()); err.clear(); };
    auto with = [&](const char* name, brov_imu_params p, int which, size_t at, double v) {
        std::vector<double> sigma(B * 12, 0.1), bias(B * 6, 0.01), drop(B, 0.5);
        if (which == 0) sigma[at] = v;
        if (which == 1) bias[at] = v;
        if (which == 2) drop[at] = v;
        report(name, im.set_host(&p, sigma.data(), bias.data(), drop.data(), nullptr, 0, nullptr, ctx));
    };
    brov_imu_params p = good;
    p.h = 0.0; with("h = 0", p, -1, 0, 0);
    p.h = -0.01; with("h < 0", p, -1, 0, 0);
    p.h = nan; with("h NaN", p, -1, 0, 0);
    p = good; p.gps_every = 0; with("gps_every = 0", p, -1, 0, 0);
    with("sigma < 0", good, 0, 17, -1e-9);
    with("sigma NaN", good, 0, B * 12 - 1, nan);
    with("bias inf", good, 1, 4, inf);
    with("bias NaN", good, 1, B * 6 - 1, nan);
    with("dropout > 1", good, 2, 1, 1.0000001);
    with("dropout < 0", good, 2, 0, -0.1);
    with("dropout NaN", good, 2, B - 1, nan);
    // the checks of a stage that is on: the step length and the index
    im.on = true; im.par.h = 0.01;
    report("dt != h", im.dt_ok(0.05 / 5, ctx) == BROV_OK ? im.dt_ok(0.010000000000000002, ctx) : 99);
    report("index 2^24", im.steps_ok((1LL << 24) - 3, 3, ctx));
    if (im.steps_ok((1LL << 24) - 3, 2, ctx) != BROV_OK || im.dt_ok(0.01, ctx) != BROV_OK) return 2;
    std::printf("waits => %d\nallocations => %d\n", waits, (int)(im.sigma != nullptr || im.out.imu != nullptr));
    return 0;
}
