"""tools/wait_audit.py's parser on a short disassembly excerpt with known waits and distances (CPU only).

tests/golden/wait_audit/excerpt.txt is hand-written in llvm-objdump's format: three functions, the middle one
(_Z6kernelILb0E...) with a prologue, one loop (the backward branch at 0x2044 to 0x2018) and an epilogue."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import wait_audit as W  # noqa: E402

TEXT = open(os.path.join(ROOT, "tests", "golden", "wait_audit", "excerpt.txt")).read()


def test_kernel_body_takes_the_named_function_only():
    body = W.kernel_body(TEXT, "_Z6kernelILb0E")
    assert len(body) == 21
    assert body[0] == W.Ins(0x2000, "s_load_dwordx2", "s[0:1], s[4:5], 0x0")
    assert body[-1].op == "s_endpgm" and body[-1].addr == 0x2068
    assert [i.op for i in W.kernel_body(TEXT, "_Z9other")] == ["s_load_dword", "s_waitcnt", "s_endpgm"]
    assert W.kernel_body(TEXT, "_Z7missing") == []


def test_loop_is_the_backward_branch():
    body = W.kernel_body(TEXT, "_Z6kernelILb0E")
    assert W.branch_target(body[13]) == 0x2018
    assert W.main_loop(body) == (4, 13)
    assert W.main_loop(W.kernel_body(TEXT, "_Z9other")) is None


def test_waits_producers_and_distances():
    body = W.kernel_body(TEXT, "_Z6kernelILb0E")
    rows, loop = W.audit(body)
    got = [(body[k].addr, region, c, v, None if p is None else body[p].op, d, o) for k, region, c, v, p, d, o in rows]
    assert got == [
        (0x200C, "pre", "lgkmcnt", 0, "s_load_dwordx2", 2, 2),
        # lgkmcnt(1) lets the newest read stay in flight: it waits for the one before it
        (0x202C, "loop", "lgkmcnt", 1, "ds_read_b32", 2, 3),
        (0x2034, "loop", "vmcnt", 0, "global_load_dword", 6, 6),
        (0x2034, "loop", "lgkmcnt", 0, "ds_read_b32", 4, 4),
        (0x2058, "post", "lgkmcnt", 0, "ds_read_b64", 3, 3),
        (0x2064, "post", "vmcnt", 0, "global_store_dwordx2", 1, 1),  # a store counts in vmcnt on gfx9
    ]


def test_report_lists_loop_and_post_and_counts_near_waits():
    body = W.kernel_body(TEXT, "_Z6kernelILb0E")
    out = io.StringIO()
    W.report(body, near=3, out=out)
    lines = out.getvalue().splitlines()
    assert "decimation loop 0x2018 .. 0x2044: 10 instructions, 48 bytes" in lines[0]
    listed = [l.split() for l in lines if not l.startswith("#")]
    assert [(l[0], l[1], l[2]) for l in listed] == [
        ("0x202c", "loop", "lgkmcnt(1)"), ("0x2034", "loop", "vmcnt(0)"), ("0x2034", "loop", "lgkmcnt(0)"),
        ("0x2058", "post", "lgkmcnt(0)"), ("0x2064", "post", "vmcnt(0)")]
    assert "# loop lgkmcnt: 2 waits, 1 within 3 instructions" in out.getvalue()
    assert "# post vmcnt: 1 waits, 1 within 3 instructions" in out.getvalue()
    assert lines[-1] == "# scalar loads inside the loop: 0"
    out = io.StringIO()
    W.report(body, show_pre=True, out=out)
    assert any(l.split()[:2] == ["0x200c", "pre"] for l in out.getvalue().splitlines())
