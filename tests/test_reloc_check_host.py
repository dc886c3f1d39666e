"""CPU check of the replica's pointer invariant (rbg_reloc_check.hpp: what replicate_finish checks on DevIndex and on every record of the pointer tables, and
what rbg_replica_pointer_check reports) on fake records, with the mistakes it exists to find planted on purpose."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reloc_check_finds_each_planted_mistake(tmp_path):
    """tests/cpp/reloc_check.cpp under ASan + UBSan.  A record of scalars, 32-bit pairs, four pointers and an array of eight (with padding) is copied and re-pointed
    member by member, as the library does it, over allocation sets of 1, 2 and 40 ranges -- the targets far from the sources, and interleaved with them in
    address as on a replica made on the same device.  A correct copy gives no violation and a pointer count equal to the non-null pointers planted (null stays
    null, uncounted).  Positive controls, each reported ALONE at its byte offset with its class: a pointer left as it was (three members), a pointer to untracked
    memory that was nulled, a pointer re-pointed into the wrong allocation / to a wrong offset / to null, a changed 64-bit scalar, half of a 32-bit pair and a
    padding byte; three at once in offset order.  First and last byte of an allocation are inside, one past the end and one before are not; two allocations
    adjacent in address keep to their own targets; strided records; a tail shorter than a word.  The line asserted counts the comparisons and the controls: a
    case that stops running changes it."""
    exe = tmp_path / "reloc"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "reloc_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout == b"reloc ok checks 138 controls 38\n", p.stdout[-600:] + p.stderr[-600:]
