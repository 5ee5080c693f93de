"""The VCFX_sample_extractor golden cases (tests/golden/sample_extractor_cases.json.gz)."""
import base64
import gzip
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_cases():
    with gzip.open(os.path.join(GOLDEN, "sample_extractor_cases.json.gz"), "rb") as f:
        cases = json.loads(f.read())["cases"]
    for c in cases:
        c["stdout"] = base64.b64decode(c["stdout"])
        c["stderr"] = base64.b64decode(c["stderr"])
    return cases


def case_stdin(case):
    """the case's stdin bytes; it runs with cwd = GOLDEN"""
    if case["stdin"]:
        with open(os.path.join(GOLDEN, case["stdin"]), "rb") as f:
            return f.read()
    return b""
