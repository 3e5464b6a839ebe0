"""csrc/host/batch_planner.hpp for_each_flat_memo_hot, the hot entries in front of the planner's memo that the fused single-term step
reads (csrc/api/fused.hpp term_batch_resident): tests/cpp/hot_memo_test.cpp, a stand-alone program, built plain and under
-fsanitize=address,undefined. No GPU, nothing loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_hot_entries_agree_with_the_memo(tmp_path, sanitize):
    exe = str(tmp_path / "hot_memo_test")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "hot_memo_test.cpp")])
    assert subprocess.check_output([exe], text=True).strip() == "hot_memo OK"
