// fleet_plant_device.hpp -- what every plant kernel of the fleet does around its integration, shared by fleet_kernel.hip (still water) and
// fleet_water_kernel.hip (moving water): where a vehicle's input comes from, the status rule, and what a step records.  The integration
// between the two halves is the kernel's own: plant_erk4 (bluerov2_model.hpp) under the tag of what is in force.  Device code.
#pragma once
#include <hip/hip_runtime.h>

#include "fleet_kernel.hpp"
#include "nmpc_device.hpp"
#include "bluerov2_model.hpp"

namespace brov {

// what the gather hands to the integration and on to the record of the step
struct FleetVehicleStep {
    double x[NX], u[NU];
    ModelPar m;
    Wrench w;
    int win, status;
};

// the input from the winner or the zero-order hold, the status rule, the vehicle's state and true parameters
__device__ __forceinline__ void fleet_plant_gather(const FleetPlantArgs& A, int v, FleetVehicleStep& s) {
    s.win = A.winner[v];
    const brov_result* __restrict__ g = A.res + (size_t)v * A.C;
    const double* usrc;
    s.status = BROV_STATUS_SUCCESS;
    if (s.win >= 0) {
        usrc = g[s.win].u0;
    } else {
        // zero-order hold: the input applied last (zeros after a reset); the status is candidate 0's, or NAN where candidate 0 reported
        // success with a cost that is not finite
        usrc = A.u_hold + (size_t)v * NU;
        const int s0 = g[0].status;
        s.status = s0 != BROV_STATUS_SUCCESS ? s0 : BROV_STATUS_NAN;
    }
    plant_inputs(A.xv + (size_t)v * NX, usrc, A.pp + (size_t)v * A.pp_stride, nullptr, 0, s.x, s.u, s.m, s.w);
}

// state / held input / status and the log rows of this tick
__device__ __forceinline__ void fleet_plant_record(const FleetPlantArgs& A, int v, const FleetVehicleStep& s) {
    store_row(A.xv + (size_t)v * NX, s.x);
    store_row(A.u_hold + (size_t)v * NU, s.u);
    A.status[v] = s.status;
    log_row(A.xlog, v, s.x);
    log_row(A.ulog, v, s.u);
    if (A.stlog) A.stlog[v] = s.status;
    if (A.winlog) A.winlog[v] = s.win;
}

// the plant step of vehicle v: gather, plant_erk4 under `ww`, record
template <class WW>
__device__ __forceinline__ void fleet_plant_vehicle(const FleetPlantArgs& A, int v, const WW& ww) {
    FleetVehicleStep s;
    fleet_plant_gather(A, v, s);
    plant_erk4(s.x, s.w, s.m, ww, A.dt, A.substeps);
    fleet_plant_record(A, v, s);
}

}  // namespace brov
