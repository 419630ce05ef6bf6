"""Completeness of tests/test_gpu_stream_order.py, checked without a GPU: every function of include/robustcap_hip.h that takes a `stream`
is called by a case of CASES or stands in EXEMPT with a reason, nothing there names an entry that no longer exists, and every case that
is let off the warm `held` condition quotes the header's own words for the synchronisation."""
import os
import re

import test_gpu_stream_order as S

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "robustcap_hip.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def _declarations(text):
    """{name: parameter list} of every `int rc_*(...)` declared in the header, comments stripped"""
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return {m.group(1): " ".join(m.group(2).split()) for m in re.finditer(r"\bint\s+(rc_\w+)\s*\(([^;{]*?)\)\s*;", code, flags=re.S)}


def _stream_entries():
    return sorted(n for n, params in _declarations(_header()).items() if re.search(r"\bvoid\s*\*\s*stream\b", params))


def test_the_parser_sees_the_header():
    decl = _declarations(_header())
    assert "rc_create" in decl and "rc_gemm_timing_busy" in decl and len(decl) > 100
    entries = _stream_entries()
    assert len(entries) >= 57, len(entries)                                # (as many when this test was written; entries are only added)
    assert "rc_step" in entries and "rc_camera_inputs_rows" in entries and "rc_live_step" not in entries and "rc_gemm_timing" not in entries


def test_every_stream_taking_entry_is_in_a_case_or_exempt():
    entries = set(_stream_entries())
    called = {e for c in S.CASES for e in c.entries}
    missing = sorted(entries - called - set(S.EXEMPT))
    assert not missing, f"entries with a stream parameter that no case calls and EXEMPT does not explain: {missing}"
    gone = sorted((called | set(S.EXEMPT)) - entries)
    assert not gone, f"named by a case or by EXEMPT, but the header declares no such stream-taking entry: {gone}"
    both = sorted(called & set(S.EXEMPT))
    assert not both, f"exempt AND called by a case: {both}"


CSRC = os.path.join(os.path.dirname(HEADER), "..", "robustcap_amd", "csrc")


def _bodies():
    """{name: body} of every `int rc_*(...) { ... }` defined at the start of a line in the library's host sources"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith(".cpp"):
            continue
        with open(os.path.join(CSRC, f)) as src:
            text = src.read()
        for m in re.finditer(r"^int (rc_\w+)\([^{;]*\)\s*\{(.*?)^\}", text, flags=re.S | re.M):
            out[m.group(1)] = m.group(2)
    return out


def test_exemptions_are_only_diagnostics_and_wrappers():
    """An exempt entry is either marked DIAGNOSTIC in the header's comment above it, or its whole body is a null check and one `return
    impl(...)` of an implementation function that an entry of some case returns too."""
    header, bodies = _header(), _bodies()
    called = {e for c in S.CASES for e in c.entries}
    impl_of = lambda body: re.findall(r"return\s+(\w+_impl)\s*\(", body)
    shared = {i for e in called for i in impl_of(bodies.get(e, ""))}
    for name, reason in S.EXEMPT.items():
        assert isinstance(reason, str) and len(reason.strip()) >= 20 and "\n" not in reason, (name, reason)
        comment = header[:header.index("int " + name + "(")].rsplit("/*", 1)[1]
        if "DIAGNOSTIC" in comment:
            continue
        body = bodies[name]
        statements = [x for x in body.split(";") if x.strip()]
        assert len(statements) == 2 and "if (!ctx) return RC_ERR_INVALID" in statements[0], (name, "more than a wrapper")
        assert impl_of(body) and impl_of(body)[0] in shared, (name, "wraps nothing that a case runs")
    assert len(S.EXEMPT) <= 4, sorted(S.EXEMPT)


def test_cases_are_well_formed():
    names = [c.name for c in S.CASES]
    assert len(names) == len(set(names))
    for c in S.CASES:
        assert c.entries and all(callable(f) for f in (c.make, c.inputs, c.call)), c.name


def test_every_case_let_off_the_held_condition_quotes_the_header():
    flat = " ".join(re.sub(r"^ \*(?= |$)", "", _header(), flags=re.M).split())       # (the comment blocks' leading " *" removed)
    for c in S.CASES:
        if c.sync is None:
            continue
        quotes = re.findall(r'"([^"]+)"', c.sync)
        assert quotes, (c.name, "no quoted clause")
        for q in quotes:
            for piece in q.split(" ... "):
                assert " ".join(piece.split()) in flat, (c.name, piece)
        assert any(e in c.sync or "Conventions" in c.sync for e in c.entries), (c.name, c.sync)
