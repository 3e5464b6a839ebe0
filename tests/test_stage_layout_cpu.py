"""csrc/host/stage_layout.hpp, the typed layout of a staged plan and the bounds-checked view of its two buffers, against the
offset rule the byte arithmetic in rgpu_api.hip followed: tests/cpp/stage_layout_test.cpp, a stand-alone program. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_layout_offsets_end_markers_and_bounded_puts(tmp_path):
    exe = str(tmp_path / "stage_layout_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "stage_layout_test.cpp")])
    assert subprocess.check_output([exe], text=True).strip() == "stage_layout OK"
