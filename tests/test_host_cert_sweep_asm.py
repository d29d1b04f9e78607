"""The single-pass search kernels read their argument block through scalar loads (kernels.hip, args_here): kernels.hip is compiled
device-only to assembly and the per-lane `flat_load`s of the four SinglePass<16, false, ., .> instantiations -- the kernels the
resident loops run -- are counted.  A flat load there is a value that is the same in all 64 lanes going through the vector L1,
the resource these kernels are bound by, and a full drain of both counters behind it.  No GPU needed; skipped without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# flat loads left on purpose, per instantiation (THRESH, COUNT, FUSE, DEFER) -> (count, reason): none.  Every place that read
# arguments behind a laundered generic pointer -- the sweep, q16_query, the certificate's address at the hand-out and at the
# retire, the pass that searches thin acceptances again -- reads them through the constant address space now, and none of them
# cost the six-wave kernels a register.
LEFT = {}


@pytest.fixture(scope="module")
def kernels_asm(tmp_path_factory):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not (os.path.isfile(hipcc) and os.access(hipcc, os.X_OK)):
        pytest.skip("no hipcc")
    out = str(tmp_path_factory.mktemp("asm") / "kernels.s")
    src = os.path.join(ROOT, "3dtk_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           "-I", src, "--cuda-device-only", "-S", os.path.join(src, "kernels.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    body, cur = {}, None
    for line in open(out):
        m = re.match(r"^_ZN4tdtk15k_search_refillINS_10SinglePassILi(\d+)ELb([01])ELi(\d+)ELb([01])EEEEEvNS_10SearchArgsE:", line)
        if m:
            cur = (int(m.group(1)), m.group(2) == "1", int(m.group(3)), m.group(4) == "1")
            body[cur] = []
        elif cur is not None:
            body[cur].append(line)
            if re.match(r"^\s*s_endpgm", line):
                cur = None
    return body


def _flat_loads(lines):
    return [i for i, l in enumerate(lines) if re.match(r"^\s*flat_load", l)]


def test_the_sweep_reads_its_arguments_through_scalar_loads(kernels_asm):
    """No flat_load between the entry of k_search_refill<SinglePass<16, false, 3, true>> and its main loop -- nor behind it: the
    kernel has none at all, and the sweep's vector loads are the slab's (global_load), its arguments s_loads."""
    lines = kernels_asm[(16, False, 3, True)]
    assert len(lines) > 3000
    assert _flat_loads(lines) == []
    assert sum(1 for l in lines if re.match(r"^\s*s_load", l)) > 100
    assert sum(1 for l in lines if re.match(r"^\s*global_load", l)) > 50


@pytest.mark.parametrize("fuse", [0, 3])
@pytest.mark.parametrize("defer", [False, True])
def test_no_flat_loads_in_the_kernels_the_loops_run(kernels_asm, fuse, defer):
    key = (16, False, fuse, defer)
    assert key in kernels_asm, sorted(kernels_asm)
    assert len(_flat_loads(kernels_asm[key])) <= LEFT.get(key, (0, ""))[0], key
