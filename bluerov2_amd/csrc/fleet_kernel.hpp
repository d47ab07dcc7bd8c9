// fleet_kernel.hpp -- launchers of the fleet planning kernels (fleet_kernel.hip) for their host side (fleet_api.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bluerov2_nmpc.h"

namespace brov {

// winner[v] = arg-min of cost over the eligible records rec[v * C .. v * C + C - 1] (index within the group, -1: none);
// winner_rec[v] (or nullptr) = a copy of that record, zeros without a winner
void launch_fleet_select(const brov_result* rec, int V, int C, int32_t* winner, brov_result* winner_rec, hipStream_t st);

// what one plant step of the fleet reads and writes; the logs are rows [V][..] of this tick or nullptr
struct FleetPlantArgs {
    int V, C;
    double* xv;                  // [V][12] vehicle states, stepped in place
    const brov_result* res;      // [V * C] records: u0 of the winner, status of candidate 0
    const int32_t* winner;       // [V]
    const double* pp;            // true parameters of vehicle v at pp + v * pp_stride
    long long pp_stride;
    double dt;
    int substeps;
    double* u_hold;              // [V][4] last applied input: read without a winner, always written
    int32_t* status;             // [V] status of this step
    double *xlog, *ulog;         // [V][12], [V][4]
    int32_t *stlog, *winlog;     // [V], [V]
};
void launch_fleet_plant(const FleetPlantArgs& a, hipStream_t st);

// the same step under the world-frame wrench wv[v][0..5] (DEVICE [V][6]), held over the tick
void launch_fleet_plant_wrench(const FleetPlantArgs& a, const double* wv, hipStream_t st);

// the same step in moving water (fleet_water_kernel.hip): under wv (nullptr: no world wrench), in the current of cg at `tick` (which may be
// OFF where the Coriolis stage is on) and with the Coriolis stage of co where its terms are not 0; the vehicle v is the generators' instance
// index.  cg.last / co.last <- the current applied / the stage's force at the start state; Gauss-Markov mode: the state advances
struct CurrentGen;
struct CoriolisGen;
void launch_fleet_plant_water(const FleetPlantArgs& a, const double* wv, const CurrentGen& cg, const CoriolisGen& co, long long tick, hipStream_t st);

// what the disturbance observer is fed per vehicle: y12[v] = xv[v], thrust[v] = allocation of u_hold[v] / kRotor, acc[v] = (v - vprev[v]) / dt;
// vprev[v] := the velocities of xv[v]
void launch_fleet_observe_inputs(int V, double dt, const double* xv, const double* u_hold, double* vprev, double* thrust, double* y12, double* acc,
                                 hipStream_t st);

// par[v * C + c][stage][0..3] = mp[v][0..3] for every candidate c and every stage; [4..15] untouched
void launch_fleet_apply(int V, int C, int stages, const double* mp, double* par, hipStream_t st);

// x0[v * C + c][:] = xv[v][:] for every candidate c
void launch_fleet_bcast(const double* xv, int V, int C, double* x0, hipStream_t st);

}  // namespace brov
