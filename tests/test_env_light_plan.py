"""What the scene plan prepares for the shade kernels' light sampling, checked without a device: tests/scene_plan/check_env_block.cpp, a program of its own built from the
plan unit and the SAH builder as tests/test_abi_and_host.py builds check_plan.cpp. It holds the environment light's uniform block (csrc/dev_scene.h: EnvUniform) against the
light's own matrices and the plan's env_marg_cdf / env_cdf / env_func_int bit for bit -- for a constant environment, for maps the register tables cannot hold, for two infinite
lights, for none -- and the record headers (type, delta bit) of a scene with one light of every kind. It passes when the program exits 0."""
import os
import subprocess


def test_env_block_and_light_headers_on_the_cpu(pkg, tmp_path):
    here = os.path.dirname(pkg.runtime.LIB_PATH)
    root = os.path.dirname(os.path.abspath(__file__))
    exe = str(tmp_path / "check_env_block")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-I", here, "-o", exe,
                           os.path.join(root, "scene_plan", "check_env_block.cpp"), os.path.join(here, "scene_plan.hip"), os.path.join(here, "host_bvh.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
