"""CPU check of the document directory (rbg_docdir.hpp: the shift rule, the builder and the lookup that rbg_docs_prepare and the kernels of k_docs.hip share)
at table sizes, start values and crowded buckets that no index of test size reaches."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_document_lookup_against_a_count_over_the_starts(tmp_path):
    """tests/cpp/docdir_check.cpp under ASan + UBSan.  Every table goes through the real builder (the size is the LAST start given + 1, the shift is the
    smallest that bounds the directory by two buckets per document); every lookup -- rank, document and offset -- is compared with a plain count of the
    starts below q = min(l + 1, size): every position of tables of 1, 2, 64 and 65 documents (equal lengths, one-symbol documents, a first start above
    0); each start, start - 1, start + 1 and 0, size - 2, size - 1, size, size + 1, 2^64 - 2, 2^64 - 1 of tables of 4096 and 2^16 documents (equal
    lengths, a first start above 0, one document holding 99 % of the text so that crowded buckets take the bisection); starts of 10 to 12 decimal
    digits up to 3e11; starts out of order with the last given start smallest, in the middle and second largest; equal starts; a last start of
    2^64 - 1 (the size wraps to 0); 4000 fixed-seed tables.  The line asserted is the number of lookups per path (an empty bucket answered by the
    directory alone, a scan of up to four candidates, the bisection of a crowded bucket): a case that stops reaching its path changes it."""
    exe = tmp_path / "docdir"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "docdir_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, timeout=300)
    assert p.returncode == 0 and b"docdir ok tables 4027 directory 1195551 scan 1437432 search 1113324\n" == p.stdout, p.stdout[-300:] + p.stderr[-600:]
