"""The A/B switch readers of csrc/common.hpp (env_set, env_int, env_int_in) on unset, empty, non-numeric, below-range,
in-range and above-range values: a stand-alone host program (tests/env_knobs_main.cpp) compiled against the header and
run.  No GPU: the program holds no kernel and makes no HIP call."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_env_readers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "env_knobs")
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function",
                    os.path.join(HERE, "env_knobs_main.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if k != "SEG3D_TEST_KNOB"}
    p = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stdout + p.stderr
