"""The flagship benchmark with the VRF audit on (RunConfig.vrf_audit): bench.py's own run and result line, the
flag set through its RunConfig override (the audit's counters are in the result's engine_stats).

    python scripts/bench_vrf_audit.py --steps 20 --warmup 5
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_vrf_audit.py --steps 20 --warmup 5

Compare with `python bench.py --steps 20 --warmup 5` on the same box (docs/PERF.md, "VRF audit")."""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

if __name__ == "__main__":
    sys.argv += ["--set", "vrf_audit=true"]
    raise SystemExit(bench.main())
