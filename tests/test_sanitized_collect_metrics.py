"""The host side of the VCF count stream (csrc/stream.hip: vcf_count_stream — reader threads, staging ring, one cleanup block)
under AddressSanitizer + UndefinedBehaviorSanitizer, on the files of tests/test_gpu_collect_metrics.py."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_vcf_count_stream_under_asan_and_ubsan():
    from snp_pipeline_amd import build
    try:
        build.build_sanitized("address", verbose=False)
        env = build.sanitized_env("address")
    except RuntimeError as e:
        if "not found" in str(e):
            pytest.skip(str(e))
        raise
    # a Python process with the HIP runtime in it never frees everything at exit: leak checking stays off, whatever the
    # environment of the caller says (build.SANITIZERS only sets a default)
    env["ASAN_OPTIONS"] = ":".join([o for o in env.get("ASAN_OPTIONS", "").split(":") if o and not o.startswith("detect_leaks=")] + ["detect_leaks=0"])
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    argv = ["-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", "-m", "gpu", "tests/test_gpu_collect_metrics.py", "-k", "small_shapes or unusual or bundled or edge or forty"]
    r = subprocess.run([sys.executable] + argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    report = "\n".join(ln for ln in (r.stdout + r.stderr).splitlines() if "Sanitizer" in ln or "runtime error" in ln)
    assert r.returncode == 0 and not report, (r.returncode, report or (r.stdout + r.stderr)[-3000:])
    assert " passed" in r.stdout and "failed" not in r.stdout
