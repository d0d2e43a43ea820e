"""Record what the single-launch C entry points do, as the JSON table that tests/test_gpu_entry_surface.py replays and compares entry by
entry (the cases, and how one is run and kept, are tests/entry_surface_cases.py):
    python tools/record_entry_surface.py [--lib PATH/libdotring_hip.so] [--out FILE]   -> tests/golden/entry_surface_gpu.json
The file was written once, by the library of the commit before the host round trips of these entry points were merged into one
(--lib), and is not regenerated: a difference is a change of behaviour.  Before it writes, the recorder checks every accepted output
that has one against the independent restatements (tests/*_ref.py, oracle/pyref, the RFC 9380 vector files) and that every covered
entry point has an accepted and a refused case; it exits non-zero, and names what differs, if either fails."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import entry_surface_cases as cases  # noqa: E402
from dot_ring_amd import _native  # noqa: E402


def coverage_gaps(table, records):
    """the covered entry points without an accepted or without a refused record"""
    accepted = {c.fn for c in table if records.get(c.key, {}).get("rc") == 0 and ("out" in records[c.key] or "launches" in records[c.key])}
    refused = {c.fn for c in table if records.get(c.key, {}).get("rc", 0) != 0}
    return [f"{fn}: no {'accepted' if fn not in accepted else 'refused'} case" for fn in cases.COVERED if fn not in accepted or fn not in refused]


def main():
    if "--lib" in sys.argv:
        _native.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else cases.GOLDEN
    table = cases.table()
    records, raws = cases.run_all(_native.lib(), table)
    launched = [c.key for c in table if records[c.key]["rc"] != 0 and "launches" in records[c.key] and c.key not in cases.REFUSED_AFTER_SW_TO_TE]
    problems = cases.check_expectations(table, raws) + coverage_gaps(table, records) + [f"{k}: refused after a launch" for k in launched]
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cases.dump_golden(records, out + (".rejected" if problems else ""))
    print(f"{out}: {len(records)} entries, library {_native.LIB_PATH}")
    if problems:
        raise SystemExit("not written as the golden file (kept beside it as .rejected):\n  " + "\n  ".join(problems))


if __name__ == "__main__":
    main()
