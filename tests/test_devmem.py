"""The owners of fb_devmem.h on the CPU: tests/devmem_host.cpp -- the real header over tests/hipstub's runtime,
a stand-alone program under g++ with the address (leak check on) and undefined-behaviour sanitizers -- checks
DevBuf / PinnedBuf, the all-or-nothing group, StreamScratch's call order and DevEvent / DevStream, and exits
non-zero at the first miss."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_owners_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "devmem_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(HERE, "hipstub"), "-o", exe,
                    os.path.join(HERE, "devmem_host.cpp")], check=True)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("devmem ok")


def test_header_is_host_only():
    with open(os.path.join(os.path.dirname(HERE), "flodbadd_amd", "csrc", "fb_devmem.h")) as f:
        lines = f.read().splitlines()
    includes = [l.split()[1] for l in lines if l.startswith("#include")]
    assert includes[0] == "<hip/hip_runtime.h>" and all(i.startswith("<") and "/" not in i for i in includes[1:])
    assert not any("__global__" in l or "__device__" in l for l in lines)
