"""CPU: the two instances of covis_kernel (connection form, vote form) exist once each in the gfx950 code object of covis.hip, use no
scratch memory and declare no static LDS: every byte a workgroup uses is in the dynamic carve that dispatch.hpp states (covis_carve),
which at SNK_COVIS_MAX_KF keyframes and SNK_COVIS_MAX_CAP entries stays inside a compute unit's 160 KiB and at 4096 keyframes with
64 entries lets at least four workgroups share one (read from the compiler's resource remarks, the method of
test_mappoint_resources.py; the carves through tests/cpp/covis_core_driver.cpp)."""
import subprocess

from test_covis_core_cpu import driver  # noqa: F401  (fixture)
from test_kernel_resources import resources


def test_covis_kernels_exist_do_not_spill_and_keep_their_lds_in_the_carve(driver):  # noqa: F811
    res = resources("covis.hip")
    for k in ("covis_kernelILb1ELb1ELb1ELb1", "covis_kernelILb0ELb0ELb0ELb0"):
        hits = {n: v for n, v in res.items() if k in n}
        assert len(hits) == 1, f"{k}: not exactly one such kernel in covis.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("LDS Size") == 0, f"{n}: static LDS beside the carve: {v}"
            # four workgroups of four wavefronts on a compute unit are four wavefronts per SIMD: the registers must allow them
            assert v.get("Occupancy") >= 4, f"{n}: {v}"
    assert len([n for n in res if "covis_kernel" in n]) == 2
    line = subprocess.run([str(driver), "--consts"], capture_output=True, text=True, check=True).stdout.split()
    k = dict(zip(line[::2], map(int, line[1::2])))
    assert k["carve_max"] <= 160 * 1024
    assert 4 * k["carve_4096_64"] <= 160 * 1024
