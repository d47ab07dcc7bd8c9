"""Which kernels a solver launches, and from which workspaces: the host's decisions row by row against tests/golden/dispatch_table.json,
recorded by scripts/make_dispatch_golden.py on the MI355X before the dispatch code was gathered into plan_workspaces / plan_solve
(nmpc_api.hip) and the kernel table (qp_kernel.hip).  Every row sits on a boundary of a rule -- horizons 4 | 11/12 | 23/24 | 47/48 |
80/81/82 | 128/129, batches around one and two instances per CU, kernel_path, uniform / general grid, rti_phase 0 and 1 -> 2, the tick
mailbox limit, brov_solve_ticks, the workspace-sizing knobs -- and every recorded field must come out equal: device_bytes, window_stages,
lds_kernel_info, last_kernel_path, the parallel-in-time kernel's count, the status vector, the return code and text of each rti_phase call.
Nothing numerical beyond status: the accuracy of each path is the business of the other GPU suites."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_dispatch_decisions_equal_the_recorded_table():
    spec = importlib.util.spec_from_file_location("make_dispatch_golden", os.path.join(ROOT, "scripts", "make_dispatch_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    import torch
    with open(m.GOLDEN) as f:
        want = json.load(f)
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    if cus != want["cus"]:
        pytest.skip(f"the table was recorded on a device with {want['cus']} CUs, this one has {cus}: the batch limits sit elsewhere")
    got = json.loads(json.dumps(m.walk()))
    diff = m.differences(want, got)
    assert not diff, "\n".join(diff[:40])
