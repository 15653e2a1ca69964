"""CPU: the kernels of snk_mappoint_refresh / snk_mappoint_refresh_batch_dev exist in the gfx950 code object of mappoint.hip, use no
scratch memory -- the packed form's row of 32 distances is sixteen statically indexed registers -- and declare no static LDS: every
byte a workgroup uses is in the dynamic carve that dispatch.hpp states (mp_packed_carve / mp_wide_carve), which for the largest
shapes stays inside a compute unit's 160 KiB and, for the packed form, lets two workgroups share one (read from the compiler's resource
remarks, the method of test_kernel_resources.py; the carves through tests/cpp/mappoint_core_driver.cpp)."""
import subprocess

from test_kernel_resources import resources
from test_mappoint_core_cpu import driver  # noqa: F401  (fixture)


def test_mappoint_kernels_exist_do_not_spill_and_keep_their_lds_in_the_carve(driver):  # noqa: F811
    res = resources("mappoint.hip")
    for k, threads in (("mp_packed_kernelILb0", 256), ("mp_packed_kernelILb1", 256), ("mp_wide_kernelILb0", 1024), ("mp_wide_kernelILb1", 1024)):
        hits = {n: v for n, v in res.items() if k in n}
        assert len(hits) == 1, f"{k}: not exactly one such kernel in mappoint.hip ({sorted(res)})"
        for n, v in hits.items():
            assert v.get("ScratchSize") == 0, f"{n}: {v}"
            assert v.get("LDS Size") == 0, f"{n}: static LDS beside the carve: {v}"
            # a 1024-thread workgroup is four wavefronts per SIMD: its registers must allow them
            assert v.get("Occupancy") >= threads // 256, f"{n}: {v}"
    line = subprocess.run([str(driver), "--forms", "0"], capture_output=True, text=True, check=True).stdout.split()
    consts = dict(zip(line[::2], map(int, line[1::2])))
    assert consts["wide_carve_max"] <= 160 * 1024 and 2 * consts["packed_carve_max"] <= 160 * 1024
