"""The 16-shape build of the hand-scheduled trunk body (tools/h3asm/gen.py, build(shape=16) -> csrc/field_h3a16_body.inc, the body of
nsff_field_kernel_h3a16): the schedule of the 32-shape body on v_mfma_f32_16x16x32_f16.  The stream passes the wait-state lint, the
functional four-wave simulator (with the instruction's operand and result lane maps, isa.py) reproduces numpy on every inference
program without the sigma ride, the committed file is the generator's output (in its compact form, whose every macro call expands to
the text of the instruction that was linted and simulated), and the default shape still produces the committed 32-shape file byte for byte.  CPU only; tests/test_h3a16_cross.py runs the assembled kernel."""
import io
import os
import sys
import contextlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "h3asm"))
import gen      # noqa: E402
import check    # noqa: E402
import isa      # noqa: E402

CSRC = os.path.join(ROOT, "nsff_pl_amd", "csrc")


def _generated(monkeypatch):
    """{file name: text} of every .inc file gen.main() writes (nothing reaches the disk)"""
    monkeypatch.setattr(sys, "argv", ["gen.py"])
    real_open = open
    written = {}

    class Sink(io.StringIO):
        def __init__(self, name):
            super().__init__()
            self.name_ = name

        def close(self):
            written[self.name_] = self.getvalue()
            super().close()

    def fake_open(path, mode="r", *a, **k):
        if "w" in mode and str(path).endswith(".inc"):
            return Sink(os.path.basename(str(path)))
        return real_open(path, mode, *a, **k)
    monkeypatch.setattr("builtins.open", fake_open)
    with contextlib.redirect_stdout(io.StringIO()):
        gen.main()
    return written


def test_committed_bodies_are_the_generators_output(monkeypatch):
    written = _generated(monkeypatch)
    assert sorted(written) == ["field_h3a16_body.inc", "field_h3a_body.inc"]
    for name, text in written.items():
        assert text == open(os.path.join(CSRC, name)).read(), f"run `python tools/h3asm/gen.py` and commit nsff_pl_amd/csrc/{name}"
    assert "v_mfma_f32_16x16x32_f16" not in written["field_h3a_body.inc"]
    defines = [ln.split()[1].split("(")[0] for ln in written["field_h3a16_body.inc"].split("\n") if ln.startswith("#define ")]
    assert defines == list(gen.MACROS16) + ["H3A16_CLOBBERS", "H3A16_BODY"]      # (nothing of the 32-shape file is defined twice)


def test_compact_form_is_the_linted_stream():
    """the committed 16-shape file spells its commonest instructions as macro calls: expanded (preprocessor string pasting, the
    assembler's register-range arithmetic), the statement is instruction for instruction the text of gen.build(shape=16)"""
    import re
    _, prog, _ = gen.build(shape=16)
    text = open(os.path.join(CSRC, "field_h3a16_body.inc")).read()
    defs = {n: (p, t) for n, p, t in re.findall(r"^#define (Q\w)\(([a-d,]+)\) (.*)$", text, re.M)}
    assert set(defs) == set(gen.MACROS16)
    body = text[text.index("#define H3A16_BODY"):].split("\n", 1)[1].replace(" \\\n", "\n")
    got = []
    for tok in re.findall(r'"(?:[^"\\]|\\.)*"|Q\w\([-\d,]*\)', body):
        if tok.startswith('"'):
            got.append(tok[1:-1])
            continue
        name, args = tok[:2], tok[3:-1].split(",")
        params, tpl = defs[name]
        piece = "".join(p[1:-1] if p.startswith('"') else args[params.split(",").index(p[1:])]
                        for p in re.findall(r'"(?:[^"\\]|\\.)*"|#[a-d]', tpl))
        got.append(re.sub(r"(\d+)\+(\d)\b", lambda m: str(int(m.group(1)) + int(m.group(2))), piece))
    want = [(i.text.replace("L_", "L_h3a_%=_") if i.kind == "label" else (i.text.replace(" L_", " L_h3a_%=_") if i.kind == "branch" else i.text)) + "\\n\\t"
            for i in prog]
    assert got == want
    assert sum(t.startswith("Q") for t in re.findall(r'"(?:[^"\\]|\\.)*"|Q\w\(', body)) > 0.7 * len(want)


def test_default_shape_is_the_32_shape_build():
    a, b = gen.build(), gen.build(shape=32)
    assert gen.render(a[0]) == gen.render(b[0]) and gen.render(a[1]) == gen.render(b[1])
    assert gen.SHAPE == 32 and gen.SAVE is False
    with pytest.raises(AssertionError):
        gen.build(save=True, shape=16)


def test_16_shape_stream_passes_the_hazard_lint():
    pre, prog, bodies = gen.build(shape=16)
    assert gen.lint(bodies, prog) == []
    assert sum(i.kind == "mfma" for i in bodies["A16R"]) == 384 and sum(i.kind == "mfma" for i in bodies["B8"]) == 192
    assert all(i.kind != "mfma" for i in pre)
    # the trunk phases multiply with the 16-shape instruction only, the HEAD phase keeps its 32x32x16 tile; no sigma ride in this build
    for name, ins in bodies.items():
        ops = {i.op for i in ins if i.kind == "mfma"}
        assert ops == ({"mfma"} if name == "HEAD" else ({"mfma16"} if ops else set())), (name, ops)
    assert "A16RS" not in bodies and "B16RS" not in bodies and "B16LP" in bodies
    # every weight slot is requested exactly once by a refilling phase, in slot order (the A phase's counted waits rely on it)
    for name in ("B16R", "B16X", "B8", "B4"):
        slots = [i.args["d"].i // 16 for i in bodies[name] if i.op == "gload_s" and i.args["d"].f == "a" and i.args["d"].i % 16 == 0]
        assert slots == list(range({"B8": 8, "B4": 4}.get(name, 16))), (name, slots)


@pytest.mark.parametrize("kind", check.KINDS16)
def test_simulated_16_shape_trunk_matches_numpy(kind):
    assert check.run_case(kind, verbose=False, shape=16) < 2e-6


def test_simulator_notices_a_missing_wait_in_the_16_shape_stream(monkeypatch):
    orig = gen.Stream.need_lds
    monkeypatch.setattr(gen.Stream, "need_lds", lambda self, tag: None if tag[0] == "xl" else orig(self, tag))
    with pytest.raises(isa.SimError, match="outstanding"):
        check.run_case("static", verbose=False, shape=16)


def test_16_shape_weights_in_the_32_shape_order_are_noticed():
    """the test of the lane maps: the 16-shape body on a 32-shape pack computes something else"""
    real = check.pack_segment
    check.pack_segment = lambda W, shape=32: real(W, 32)
    try:
        with pytest.raises(AssertionError):
            check.run_case("noskip", verbose=False, shape=16)
    finally:
        check.pack_segment = real
