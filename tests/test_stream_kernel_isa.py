"""Register budget of the persistent ensemble kernel, read off the gfx950 code object metadata (no GPU needed): the
instantiations the benchmark configurations run keep every value in registers -- no VGPR spill, no scratch memory -- and
the headline one (d = 10, four point pairs per lane) spills no SGPR into VGPR lanes either: a spilled scalar is read
back with v_readlane on the dependent chain of half steps."""
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
    out = tmp_path_factory.mktemp("isa") / "ens_stream.s"
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--offload-device-only", "-S",
           os.path.join(CSRC, "ens_stream.hip"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    text = out.read_text()
    kernels = {}
    for block in text.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        kernels[name.group(1)] = {k: int(v) for k, v in re.findall(
            r"\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", block)}
    return kernels


def _stream_kernel(d, ppt, tmax, generic):
    return "_ZN5alabi17ens_stream_kernelILi%dELi%dELi%dELb%dEEEvNS_10StreamArgsE" % (d, ppt, tmax, int(generic))


@pytest.mark.parametrize("d,ppt", [(10, 4), (5, 1), (2, 1)])
def test_benchmark_instantiations_keep_everything_in_registers(metadata, d, ppt):
    name = _stream_kernel(d, ppt, 384, False)
    assert name in metadata, "instantiation missing from the code object: " + name
    m = metadata[name]
    print(name, m)
    assert m["vgpr_spill_count"] == 0
    assert m["private_segment_fixed_size"] == 0
    assert m["vgpr_count"] <= 256


def test_headline_instantiation_spills_no_scalar(metadata):
    m = metadata[_stream_kernel(10, 4, 384, False)]
    print(m)
    assert m["sgpr_spill_count"] == 0
