"""The built library's k_rollout_q<1,*>: no role's step loop loads its constants (they are loaded once per launch, in front of
the loop), and every role loop holds two barriers.  Read off the disassembly of the gfx950 code object by
tools/quad_resident_isa.py --so; needs the compiler's tools, no GPU.  Loads and barriers only."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import REPO


def test_no_scalar_load_in_a_role_loop_and_two_barriers_each():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc is not installed")
    from f16_mpc_oop_py_amd import lib
    assert os.path.exists(lib.SO_PATH), "build() has not run"
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "quad_resident_isa.py"), "--so", lib.SO_PATH],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    rows = re.findall(r"k_rollout_q<1,(\d),(\d)> (wave \d)[^:]*: s_load (\d+) s_barrier (\d+)", r.stdout)
    assert len(rows) == 16, r.stdout                                   # four instantiations x four role loops
    assert all(int(n) == 0 and int(b) == 2 for _, _, _, n, b in rows), r.stdout
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS")
