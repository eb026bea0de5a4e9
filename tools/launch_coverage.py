"""Launch-site coverage: which of the library's kernel launch sites does a run reach?  (CPU-only.)

A run with ``DC_LAUNCH_COVERAGE_FILE=<file>`` set ("Launch sites") appends, per process, one
``site \\t test id at the site's first launch`` line for every site it reached.  This tool merges such a file with the
library's own list of sites (``_lib.launch_sites()``, host data: no GPU needed):

    python tools/launch_coverage.py <file> [--json tests/golden/launch_reach.json] [--unreached out.txt]

It writes ``{site: [test ids that first reached it, one per process]}`` for EVERY site (an empty list: never reached)
as JSON, prints the unreached sites grouped by source file, and with ``--unreached`` writes that listing to a file.
Lines of the coverage file that name no current site (a stale file) are an error.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUTSIDE = "(outside a test)"


def test_id(raw: str) -> str:
    """PYTEST_CURRENT_TEST ("tests/a.py::test_x[1] (call)") -> "tests/a.py::test_x[1]"; unset -> OUTSIDE."""
    raw = raw.strip()
    for phase in (" (setup)", " (call)", " (teardown)"):
        if raw.endswith(phase):
            raw = raw[:-len(phase)]
    return raw or OUTSIDE


def merge(coverage_path: str, sites) -> dict:
    reach = {s: [] for s in sites}
    with open(coverage_path) as f:
        for line in f:
            line = line.rstrip("\n")
            if not line:
                continue
            site, _, raw = line.partition("\t")
            if site not in reach:
                raise SystemExit(f"{coverage_path}: '{site}' is not a launch site of this library (stale file?)")
            t = test_id(raw)
            if t not in reach[site]:
                reach[site].append(t)
    return {s: sorted(v) for s, v in sorted(reach.items())}


def unreached_text(reach: dict, files: dict) -> str:
    by_file = {}
    for site, tests in reach.items():
        if not tests:
            by_file.setdefault(files[site], []).append(site)
    n = sum(len(v) for v in by_file.values())
    lines = [f"{n} of {len(reach)} launch sites not reached"]
    for src in sorted(by_file):
        lines.append(f"\n{src} ({len(by_file[src])})")
        lines += [f"  {s}" for s in sorted(by_file[src])]
    return "\n".join(lines) + "\n"


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("coverage_file")
    ap.add_argument("--json", default=os.path.join(ROOT, "tests", "golden", "launch_reach.json"))
    ap.add_argument("--unreached", default=None, help="also write the listing of unreached sites here")
    a = ap.parse_args(argv)
    from deformcontact_amd import _lib
    files = _lib.launch_site_files()
    reach = merge(a.coverage_file, list(files))
    with open(a.json, "w") as f:
        json.dump(reach, f, indent=0, sort_keys=True)
        f.write("\n")
    text = unreached_text(reach, files)
    sys.stdout.write(text)
    if a.unreached:
        os.makedirs(os.path.dirname(os.path.abspath(a.unreached)), exist_ok=True)
        with open(a.unreached, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
