"""The flagship benchmark under a --kzg-audit mode (RunConfig.kzg_audit): bench.py's own run and result line, the
mode set through its RunConfig override (the audit's counters are in the result's engine_stats).

    python scripts/bench_kzg_shares.py --mode shares --steps 100 --warmup 10
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_kzg_shares.py --mode shares --steps 40 --warmup 5

Run the modes off | consistent | shares alternately on one box and compare (docs/PERF.md, "Per-worker verifySecret
audit"); k_kzg_rows in the kernel statistics is the row kernel's own time."""
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

if __name__ == "__main__":
    mode = "shares"
    if "--mode" in sys.argv:
        i = sys.argv.index("--mode")
        mode = sys.argv[i + 1]
        del sys.argv[i:i + 2]
    if mode not in ("off", "consistent", "literal", "shares"):
        raise SystemExit(f"--mode {mode!r}: expected off | consistent | literal | shares")
    sys.argv += ["--set", f"kzg_audit={mode}"]
    raise SystemExit(bench.main())
