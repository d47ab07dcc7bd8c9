/* bluerov2_nmpc_water.h -- the water a fleet's vehicles move in: brov_vehicle_current_* and brov_vehicle_coriolis_*, the ocean current and the
 * Coriolis stage of the plant (brov_current_*, brov_coriolis_* of bluerov2_nmpc.h) at batch V, owned by a brov_fleet, the vehicle as instance
 * index.  Part of the C ABI of bluerov2_nmpc.h, which includes this file inside its fleet section (and documents the two families there);
 * not meant to be included on its own. */
#ifndef BLUEROV2_NMPC_WATER_H_
#define BLUEROV2_NMPC_WATER_H_
#ifndef BLUEROV2_NMPC_H_
#error "include bluerov2_nmpc.h, which includes this file"
#endif

int brov_vehicle_current_constant_host(brov_fleet* f, const double* v /*[V][3]*/);
int brov_vehicle_current_table_host(brov_fleet* f, const double* tab /*[rows][3]*/, int rows, const double* gain /*[V] or NULL*/);
int brov_vehicle_current_gauss_markov_host(brov_fleet* f, uint64_t seed, const double* mean /*[V][3]*/, const double* mu /*[3]*/,
                                           const double* amp /*[3]*/, const double* lo /*[3]; NULL: -5*/, const double* hi /*[3]; NULL: 5*/,
                                           double step /*seconds per tick*/);
int brov_vehicle_current_off(brov_fleet* f);
int brov_vehicle_current_mode(const brov_fleet* f);                            /* BROV_CURRENT_*; OFF for NULL */
/* the current of every vehicle at `tick` in CONSTANT / TABLE mode (zeros while OFF); moves nothing; refused in GAUSS_MARKOV mode */
int brov_vehicle_current_eval_host(brov_fleet* f, int64_t tick, double* v /*[V][3]*/);
int brov_vehicle_current_get_state_host(brov_fleet* f, double* v /*[V][3]*/);  /* what the next fleet step applies */
int brov_vehicle_current_set_state_host(brov_fleet* f, const double* v /*[V][3]*/);   /* GAUSS_MARKOV only */
int brov_vehicle_current_last_host(brov_fleet* f, double* v /*[V][3]*/);       /* of the last fleet step in a current (zeros before the first and after a reset) */
int brov_vehicle_coriolis_set(brov_fleet* f, int terms /*1..3*/, double ka, double ma);
int brov_vehicle_coriolis_off(brov_fleet* f);
int brov_vehicle_coriolis_terms(const brov_fleet* f);                          /* the bit mask in force; 0 for NULL or off */
int brov_vehicle_coriolis_get(const brov_fleet* f, int* terms, double* ka, double* ma);   /* as last set (terms 0 while off; before any set: 0, 0, 1.2481) */
/* the force alone, c = [X Y Z N] per vehicle, at the states x in water moving with vc (NULL: still water), with the terms in force (off:
 * zeros) and the parameters the next fleet step would read.  Moves nothing */
int brov_vehicle_coriolis_eval_host(brov_fleet* f, const double* x /*[V][12]*/, const double* vc /*[V][3] or NULL*/, double* c /*[V][4]*/);
int brov_vehicle_coriolis_last_host(brov_fleet* f, double* c /*[V][4]*/);     /* at the start state of the last fleet step under the stage (zeros before the first and after a reset) */

#endif
