"""CPU: snake_hip::MapPointRefresher of the C++ adaptor header compiles (plain g++, -Wall -Werror) against the mock Keyframe / MapPoint
structs of tests/cpp/mappoint_driver.cpp and links into the driver of tests/test_cpp_mappoint_gpu.py; without inputs the driver fails
cleanly (exception text, status 1) instead of crashing."""
import subprocess

from test_cpp_mappoint_gpu import build_driver


def test_mappoint_driver_compiles_and_fails_cleanly_without_inputs(tmp_path):
    exe = build_driver(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 1 and "mappoint_driver: missing input" in r.stderr
