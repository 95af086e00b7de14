#!/usr/bin/env python3
"""On the GPU box: bench.py under alternating builds of the library, one JSON line per run (the format of profiles/chains_ab.jsonl).

usage: tools/bench_ab.py [--leg=<name>] <tag> <reps> <out.jsonl> "<build name>=<library path>" ["<build name>=<library path>" ...] [-- bench args ...]

Every run is a fresh process (`KVZ_HIP_LIB=<library> python bench.py --steps 5 --warmup 2 <bench args>`) under a time limit; the builds alternate within a repetition,
so that drift of the box lands on all of them alike.  The first run that fails, or whose result does not say `"verified": true` (bench.py checks its outputs under --full and in the --only legs: give `--full --no-extra`
behind `--`), ends the script with its status.  KVZ_AB_NO_VERDICT_OK=1 lets `"verified": null` pass: what bench.py says where it has no digests of the reference
encoder to compare with (a QP other than 22).  --leg=<name> compares an auxiliary leg's value instead of the headline's (`chain_full`: give `--full` behind `--`); a leg that says `"verified": false` ends the script like the headline.  Afterwards:
the median ratio of every build against the first one, each build's spread ((max - min) / median), and whether the slowest run of a build beats the fastest of the
first -- the project's bar is a median ratio above 1 + 5 x the first build's spread together with that."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    argv = sys.argv[1:]
    extra = []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    leg = None
    if argv[0].startswith("--leg="):
        leg, argv = argv[0][len("--leg="):], argv[1:]
    tag, reps, out = argv[0], int(argv[1]), argv[2]
    builds = [a.split("=", 1) for a in argv[3:]]
    limit = int(os.environ.get("KVZ_AB_TIMEOUT", "240"))
    values = {name: [] for name, _ in builds}
    with open(out, "a") as fh:
        for rep in range(reps):
            for name, lib in builds:
                env = dict(os.environ, KVZ_HIP_LIB=os.path.abspath(lib))
                cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "5", "--warmup", "2"] + extra
                r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
                if r.returncode != 0:
                    print(f"{tag} rep {rep} {name}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}", flush=True)
                    return r.returncode
                d = json.loads(r.stdout.strip().splitlines()[-1])
                rec = {"tag": tag, "rep": rep, "bench_args": extra, "build": name, "value": d["value"], "ms_per_step": d.get("ms_per_step"), "steps": 5, "warmup": 2,
                       "unit": d.get("unit"), "verified": d.get("verified")}
                if leg:
                    if not d.get(leg, {}).get("value"):
                        print(f"{tag} rep {rep} {name}: no leg {leg} in the result: {d.get(leg)}", flush=True)
                        return 4
                    rec.update(leg=leg, headline=d["value"], value=d[leg]["value"], leg_verified=d[leg].get("verified"))
                    d = dict(d, value=rec["value"], verified=False if d[leg].get("verified") is False else d.get("verified"))
                fh.write(json.dumps(rec) + "\n")
                fh.flush()
                print(f"{tag} rep {rep} {name}: {d['value']:.0f} {d.get('unit')} verified={d.get('verified')}", flush=True)
                if d.get("verified") is False or (d.get("verified") is None and not os.environ.get("KVZ_AB_NO_VERDICT_OK")):
                    return 3
                values[name].append(d["value"])
    base = builds[0][0]
    spread = lambda v: (max(v) - min(v)) / statistics.median(v)  # noqa: E731
    for name, _ in builds:
        v = values[name]
        line = f"{tag} {name}: median {statistics.median(v):.0f} spread {100 * spread(v):.3f} %"
        if name != base:
            line += f" ratio {statistics.median(v) / statistics.median(values[base]):.4f} slowest beats the fastest of '{base}': {min(v) > max(values[base])}"
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
