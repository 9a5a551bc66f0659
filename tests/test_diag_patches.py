"""The text patches of tools/diag/patch_build.py still apply: every substitution's pattern occurs in
its source file exactly `count` times (what build_diag checks before it builds). No build, no GPU."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _patch_build():
    spec = importlib.util.spec_from_file_location("patch_build", os.path.join(ROOT, "tools", "diag", "patch_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_diag_pattern_matches_its_count():
    pb = _patch_build()
    assert pb.DIAGS
    texts = {}
    bad = {}
    for name, subs in pb.DIAGS.items():
        assert subs, f"diag {name} has no substitution"
        for fname, old, new, count in subs:
            path = os.path.join(pb.build.CSRC, fname)
            if fname not in texts:
                texts[fname] = open(path).read() if os.path.exists(path) else None
            found = -1 if texts[fname] is None else texts[fname].count(old)  # -1: no such file
            if found != count or count < 1 or old == new:
                bad.setdefault(name, []).append(f"{fname}: found {found}x, expected {count}x: {old[:60]!r}")
    assert not bad, "diagnostics that no longer apply: " + ", ".join(sorted(bad)) + "\n" + "\n".join(
        f"  {n}: {m}" for n in sorted(bad) for m in bad[n])
