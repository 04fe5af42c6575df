"""The host half of the late-actions step without a GPU: tests/host/late_actions_main.cpp (a program of its own around
csrc/late_actions.hpp: copy-and-tag round trips, tag alternation per set, alignment and odd sizes) built with the address and
undefined-behaviour sanitizers and run on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("opt", ("-O1", "-O3"))
def test_copy_and_tag_routine_under_the_sanitizers(tmp_path, opt):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = tmp_path / "late_actions_main"
    subprocess.check_call([cxx, "-std=c++17", opt, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-I", os.path.join(ROOT, "aircombat-selfplay_amd", "csrc"), os.path.join(ROOT, "tests", "host", "late_actions_main.cpp"),
                           "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "late actions host checks ok" in run.stdout

