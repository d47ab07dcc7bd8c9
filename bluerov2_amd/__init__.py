"""bluerov2_amd -- MI355X-native batched NMPC (SQP-RTI) solver for the BlueROV2 OCP.

The compute path is the HIP library bluerov2_amd/lib/libbluerov2_nmpc.so (C ABI: include/bluerov2_nmpc.h).  This package
is the thin host-side mirror of that ABI; there is no CPU or PyTorch fallback -- without the library or without a GPU the
solver raises.
"""
from .solver import (BatchSolver, SolverOptions, RESULT_DTYPE, P_NOMINAL, build_library, library_path,  # noqa: F401
                     NoDeviceError, thrust_allocation, PATH_AUTO, PATH_STREAMING, PATH_FUSED, PATH_WINDOWED,
                     WRENCH_OFF, WRENCH_CONSTANT, WRENCH_PERIODIC, WRENCH_TABLE,
                     CURRENT_OFF, CURRENT_CONSTANT, CURRENT_TABLE, CURRENT_GAUSS_MARKOV, current_from_angles, rotor_coeffs,
                     CORIOLIS_RIGID, CORIOLIS_ADDED, ImuParams, IMU_GPSV_ELAPSED, RangeParams, InspectParams,
                     INSPECT_STATE_DTYPE, INSPECT_STATS_DTYPE, INSPECT_SHARED_PID, INSPECT_FLOAT_YAW, RANGE_MAX_BOXES, MeshInfo, load_stl, MESH_MAX_TRIANGLES,
                     CurveParams, curve_from_pwm_table, inverse_table, CURVE_LINEAR, CURVE_BASIC, CURVE_DEADZONE, CURVE_TABLE,
                     CURVE_PRE_NONE, CURVE_PRE_POLY, CURVE_PRE_TABLE, CURVE_PART_COMMAND, CURVE_PART_THRUST, CURVE_PART_BOTH,
                     CURVE_WHICH_CURVE, CURVE_WHICH_PRE, CURVE_MAX_KNOTS)

from .ekf import BatchEkf, EkfParams  # noqa: F401,E402
from .eskf import BatchEskf, EskfParams, closed_loop_eskf  # noqa: F401,E402
from .rls import BatchRls, RlsParams, APPLY_DISTURBANCE, APPLY_MODEL  # noqa: F401,E402
from .track import BatchTrack, TrackParams, TRACK_STATS_DTYPE  # noqa: F401,E402
from .fleet import Fleet  # noqa: F401,E402
from .group import SolverGroup, GATHER_RECORDS, GATHER_PACKED, rccl_version, unique_id  # noqa: F401,E402

__all__ = ["SolverGroup", "GATHER_RECORDS", "GATHER_PACKED", "rccl_version", "unique_id", "BatchEkf", "EkfParams", "BatchEskf", "EskfParams", "BatchRls", "RlsParams", "BatchTrack", "TrackParams", "TRACK_STATS_DTYPE", "Fleet", "APPLY_DISTURBANCE", "APPLY_MODEL", "BatchSolver", "SolverOptions", "RESULT_DTYPE", "P_NOMINAL", "build_library", "library_path",
           "NoDeviceError", "thrust_allocation", "PATH_AUTO", "PATH_STREAMING", "PATH_FUSED", "PATH_WINDOWED",
           "WRENCH_OFF", "WRENCH_CONSTANT", "WRENCH_PERIODIC", "WRENCH_TABLE",
           "CURRENT_OFF", "CURRENT_CONSTANT", "CURRENT_TABLE", "CURRENT_GAUSS_MARKOV", "current_from_angles", "rotor_coeffs", "CORIOLIS_RIGID", "CORIOLIS_ADDED",
           "ImuParams", "IMU_GPSV_ELAPSED", "closed_loop_eskf", "RangeParams", "InspectParams", "INSPECT_STATE_DTYPE", "INSPECT_STATS_DTYPE",
           "INSPECT_SHARED_PID", "INSPECT_FLOAT_YAW", "RANGE_MAX_BOXES", "MeshInfo", "load_stl", "MESH_MAX_TRIANGLES",
           "CurveParams", "curve_from_pwm_table", "inverse_table", "CURVE_LINEAR", "CURVE_BASIC", "CURVE_DEADZONE", "CURVE_TABLE",
           "CURVE_PRE_NONE", "CURVE_PRE_POLY", "CURVE_PRE_TABLE", "CURVE_PART_COMMAND", "CURVE_PART_THRUST", "CURVE_PART_BOTH",
           "CURVE_WHICH_CURVE", "CURVE_WHICH_PRE", "CURVE_MAX_KNOTS"]
