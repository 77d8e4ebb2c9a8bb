"""The fixture files that a reference-minted commit_ct digest pins (tests/golden/ref/manifest.json,
chainf_manifest.json, tests/golden/recrypt/manifest.json), shared by the commit_ct tests."""
import json
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture_cases():
    """(path, with_sigma, digest hex) of every fixture file pinned by a reference commit_ct digest."""
    ref, rc = os.path.join(GOLD, "ref"), os.path.join(GOLD, "recrypt")
    man = json.load(open(os.path.join(ref, "manifest.json")))
    cases = []
    for p, pair in enumerate(man["pairs"]):
        cases.append((os.path.join(ref, f"pair{p}_add.ct"), True, pair["commit_add"]))
        cases.append((os.path.join(ref, f"pair{p}_sub.ct"), True, pair["commit_sub"]))
    cases.append((os.path.join(ref, "pair0_mul.ct"), True, man["pairs"][0]["commit_mul"]))
    cases.append((os.path.join(ref, "guard_add.ct"), True, man["guard"]["commit"]))
    for k in json.load(open(os.path.join(rc, "manifest.json")))["cases"]:
        if k["sigma"]:
            cases.append((os.path.join(rc, k["name"] + "_out.ct"), True, k["commit"]))
    chain = json.load(open(os.path.join(ref, "chainf_manifest.json")))
    cases.append((os.path.join(ref, "chainf_final.ct"), False, chain["steps"][3]["commit_weights"]))
    return man, cases
