"""Register budget of the pair variant of the persistent ensemble kernel (ens_pair_kernel), read off the gfx950 code object
metadata (no GPU needed): the instantiations that the benchmark configurations C1, C2 and C3 launch are there, and no
instantiation that the library contains -- the launch table compiles exactly those that the fit rule (ens_stream_max_db) can
select -- spills a register or uses scratch memory."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "alabi_amd", "csrc")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.fixture(scope="module")
def metadata(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc is not installed")
    out = tmp_path_factory.mktemp("isa") / "ens_pair.s"
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--offload-device-only", "-S",
           os.path.join(CSRC, "ens_pair.hip"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    kernels = {}
    for block in out.read_text().split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        kernels[name.group(1)] = {k: int(v) for k, v in re.findall(
            r"\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", block)}
    return kernels


def _pair_kernel(d, ppt, tmax, generic):
    return "_ZN5alabi15ens_pair_kernelILi%dELi%dELi%dELb%dEEEvNS_8PairArgsE" % (d, ppt, tmax, int(generic))


# C3: d = 10, N = 2000 (four point pairs per lane); C2: d = 5; C1: d = 2 (one pair per lane)
@pytest.mark.parametrize("d,ppt", [(10, 4), (5, 1), (2, 1)])
def test_benchmark_instantiations_spill_nothing(metadata, d, ppt):
    name = _pair_kernel(d, ppt, 384, False)
    assert name in metadata, "instantiation missing from the code object: " + name
    m = metadata[name]
    print(name, m)
    assert m["sgpr_spill_count"] == 0
    assert m["vgpr_spill_count"] == 0
    assert m["private_segment_fixed_size"] == 0


def test_no_instantiation_spills(metadata):
    pair = {name: m for name, m in metadata.items() if "ens_pair_kernel" in name}
    assert _pair_kernel(10, 4, 384, False) in pair
    assert len(pair) == 102      # the rows of the launch table: 55 squared-exponential, 47 generic
    for name, m in pair.items():
        assert m == {"sgpr_spill_count": 0, "vgpr_spill_count": 0, "private_segment_fixed_size": 0}, (name, m)
