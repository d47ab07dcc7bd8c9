// fleet_water_kernel.hip -- the fleet's plant in moving water (include/bluerov2_nmpc.h, brov_vehicle_current_*, brov_vehicle_coriolis_*;
// DESIGN.md section 4.12c): fleet_plant_kernel / fleet_plant_wrench_kernel with the two stages that describe the water, the ocean current
// (current_gen.hpp) and the Coriolis stage (coriolis_force, plant_stages.hpp), indexed by the VEHICLE.  One lane per vehicle, blocks of 128:
//   gather (fleet_plant_gather, shared with the still-water kernels) -> the vehicle's world wrench of the tick from the buffer
//   wrench_eval_kernel wrote (WR) -> current_at(cg, v, tick) into the source's `last` -> the Coriolis force at the start state into its
//   `last` (CO) -> plant_erk4 under WorldWrenchCurrent, or WorldWrenchCurrentCoriolis (CO) -> record (fleet_plant_record) -> Gauss-Markov advance.
// The current is evaluated here: it adds no launch to a tick.  The wrench keeps its evaluation launch, whose output is the log row.
//
// What is a template parameter: the wrench <WR> and the Coriolis stage <CO>; the current's mode is run-time.  Instructions from the gfx950
// assembly listing, registers from the backend's resource report (profiles/fleet_water_isa.txt):
//   WR   without it the world wrench is six literal zeros and its projection at the four RK stages folds away, as in plant_current.hip and
//        plant_coriolis.hip: <false, false> 1489 instructions and 193 VGPRs against <true, false> 1547 and 211; <false, true> 2045 and 238
//        against <true, true> 2086 and 250.  Decided at run time (wv == nullptr: zeros) every step carries the projection: 1533 / 2096
//        instructions and 211 / 250 VGPRs with or without a wrench.  A small gain, 44 instructions of 1533; it costs two more instantiations
//        of a kernel that is small beside the solve, and follows what the two solver files do.
//   CO   picks the TAG plant_erk4 runs under, which is a type: with the current alone the vehicle integrates the code of
//        plant_current_kernel's model (third tag), with the stage that of plant_coriolis_kernel's (fourth tag), so a fleet of C = 1 steps as
//        a solver of batch V under the same settings does.  One kernel under the fourth tag with terms = 0 would carry the stage's products
//        through every step in a current alone: 2045 instructions and 238 VGPRs against 1489 and 193.
//   mode run-time, as plant_coriolis.hip settled: OFF gives zeros, and a zero current changes no bit of a finite state (v - 0 is exact), so
//        <., true> serves the Coriolis stage in still water too.  Four instantiations, not sixteen.
// Resources: 193 / 211 VGPRs without the stage, 238 / 250 with it, no AGPRs, scratch 0, LDS 0, occupancy 2 waves per SIMD for all four (the
// still-water fleet_plant_wrench_kernel sits at occupancy 2 as well); coriolis_force's selects keep the fourth tag off the 255-VGPR cliff
// here as there.
// FP64, no LDS, no scratch, no atomics.
#include <hip/hip_runtime.h>

#include "fleet_kernel.hpp"
#include "fleet_plant_device.hpp"   // fleet_plant_gather, fleet_plant_record
#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"
#include "plant_stages.hpp"   // coriolis_force, water_velocity
#include "current_gen.hpp"    // current_at, current_advance

namespace brov {

// WR: under the world wrench wv[v][0..5] of this tick; else a zero world wrench, which folds away (wv is not read).  CO: the Coriolis stage
// `co` is on.  cg: the current in force, which may be OFF under CO (then cg.last is not written: it exists only once a current was set).
template <bool WR, bool CO>
__global__ __launch_bounds__(128) void fleet_plant_water_kernel(FleetPlantArgs A, const double* __restrict__ wv, CurrentGen cg, CoriolisGen co,
                                                                long long tick) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= A.V) return;
    FleetVehicleStep s;
    fleet_plant_gather(A, v, s);
    WorldWrenchCurrent wc = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, 0.0, 0.0, 0.0};
    if constexpr (WR) {
        const double* __restrict__ w6 = wv + (size_t)v * 6;
        wc.ww = {w6[0], w6[1], w6[2], w6[3], w6[4], w6[5]};   // held over the tick
    }
    double vc[3];
    current_at(cg, v, tick, vc);   // OFF: zeros
    wc.vx = vc[0]; wc.vy = vc[1]; wc.vz = vc[2];   // held over the tick
    if (cg.mode != BROV_CURRENT_OFF) store_row(cg.last + (size_t)v * 3, vc);
    if constexpr (CO) {
        const double* __restrict__ pp = A.pp + (size_t)v * A.pp_stride;
        WorldWrenchCurrentCoriolis wcc;
        wcc.wc = wc;
        wcc.cs = {co.terms, pp[4], pp[5], pp[6], co.ka, co.ma};
        {   // the stage's force at the start state, as coriolis_eval_kernel gives it
            double c[4], nr[3] = {s.x[6], s.x[7], s.x[8]};
            if (cg.mode != BROV_CURRENT_OFF) water_velocity(s.x, vc, nr);
            const double nu[6] = {s.x[6], s.x[7], s.x[8], s.x[9], s.x[10], s.x[11]};
            coriolis_force(wcc.cs, nu, nr, c);
            store_row(co.last + (size_t)v * 4, c);
        }
        plant_erk4(s.x, s.w, s.m, wcc, A.dt, A.substeps);
    } else {
        plant_erk4(s.x, s.w, s.m, wc, A.dt, A.substeps);
    }
    fleet_plant_record(A, v, s);
    if (cg.mode == BROV_CURRENT_GAUSS_MARKOV) current_advance(cg, v, tick, vc);
}

void launch_fleet_plant_water(const FleetPlantArgs& a, const double* wv, const CurrentGen& cg, const CoriolisGen& co, long long tick,
                              hipStream_t st) {
    const dim3 grid((unsigned)((a.V + 127) / 128)), block(128);
    const bool wr_on = wv != nullptr, co_on = co.terms != 0;
#define BROV_LAUNCH_FLEET_WATER(WR, CO) hipLaunchKernelGGL((fleet_plant_water_kernel<WR, CO>), grid, block, 0, st, a, wv, cg, co, tick)
    if (wr_on && co_on) BROV_LAUNCH_FLEET_WATER(true, true);
    else if (wr_on) BROV_LAUNCH_FLEET_WATER(true, false);
    else if (co_on) BROV_LAUNCH_FLEET_WATER(false, true);
    else BROV_LAUNCH_FLEET_WATER(false, false);
#undef BROV_LAUNCH_FLEET_WATER
}

}  // namespace brov
