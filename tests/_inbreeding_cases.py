"""The VCFX_inbreeding_calculator golden cases (tests/golden/inbreeding_cases.json.gz)."""
import base64
import gzip
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cases():
    with gzip.open(os.path.join(GOLDEN, "inbreeding_cases.json.gz"), "rb") as f:
        cases = json.loads(f.read())["cases"]
    for c in cases:
        c["stdout"] = base64.b64decode(c["stdout"])
        c["stderr"] = base64.b64decode(c["stderr"])
    return cases


def case_input(case, tmp_path):
    """(stdin bytes, cwd) of a case; a synthetic case's input is generated into tmp_path"""
    if case["synth"]:
        from vcfx_amd import synth
        cfg = case["synth"]
        buf = synth.generate(*cfg[:8], format_mode=cfg[8])
        (tmp_path / "synth.vcf").write_bytes(buf)
        return (b"" if "-i" in case["argv"] else buf), str(tmp_path)
    if case["stdin"]:
        with open(os.path.join(GOLDEN, case["stdin"]), "rb") as f:
            return f.read(), GOLDEN
    return b"", GOLDEN
