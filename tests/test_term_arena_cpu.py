"""csrc/host/term_arena.hpp, the host-side bookkeeping of the device-resident term descriptors, and the planner memo that names
them (for_each_flat_memo_placed): tests/cpp/term_arena_test.cpp, a stand-alone program. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_term_arena_generations_slots_and_upload_sequences(tmp_path):
    exe = str(tmp_path / "term_arena_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "term_arena_test.cpp")])
    assert subprocess.check_output([exe], text=True).strip() == "term_arena OK"
