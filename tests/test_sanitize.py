"""libcda's host planners (celestia-app_amd/csrc/plan.cpp) under AddressSanitizer + UndefinedBehaviorSanitizer,
checked against the naive restatements in tests/san/plan_check.cpp (CPU only; scripts/sanitize.sh adds the
sanitized oracle under the whole CPU suite and keeps the log under profiles/), and the proof calls' carve helper and
workspace layouts (csrc/arena.h, the features' headers) under the same sanitizers, bound to exact-size heap buffers by
tests/san/arena_check.cpp.  Both are stand-alone programs."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_planners_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "san", "plan_check.cpp"),
                           os.path.join(ROOT, "celestia-app_amd", "csrc", "plan.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "plan_check: all passed" in out.stdout


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_proof_workspace_layouts_under_asan_ubsan(tmp_path):
    """The carve helper (csrc/arena.h) and the three proof workspaces' layouts (csrc/share_proof.h, namespace_proof.h,
    befp.h) bound to heap buffers of exactly their measured size and written through: tests/san/arena_check.cpp.  The
    layouts take their structs from headers that need HIP's, so the host compiler is hipcc's; no device code is built
    and no device touched."""
    exe = str(tmp_path / "arena_check")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "--offload-host-only", "-Xarch_host",
                           "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "san", "arena_check.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "arena_check: all passed" in out.stdout
