"""A/B of two library builds over any bench commands, the arms alternating, one child process per run:

    python scripts/ab_libs.py OUT.jsonl REPS name="python scripts/bench_policy.py --net qnet" ...

build/libmagent_parent.so (the other build, e.g. the parent commit's library copied there) against build/libmagent.so,
selected per child with MAGENT_LIB.  Every JSON line a child prints is appended to OUT.jsonl as {"bench", "lib",
"lib_sha256_16", "rep", "result"}.  Stops at the first child that fails (profiles/policy_act_ab.jsonl was made by it).
Limits: every child gets the same 240 s time limit, and a command is split at whitespace (str.split), so it cannot
carry quoted arguments or arguments with spaces."""
import hashlib, json, os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = os.path.join(REPO, "mean-field-multi-agent-reinforcement-learning_amd", "build")
LIBS = {"parent": os.path.join(B, "libmagent_parent.so"), "new": os.path.join(B, "libmagent.so")}
SHA = {k: hashlib.sha256(open(v, "rb").read()).hexdigest()[:16] for k, v in LIBS.items()}
out, reps = sys.argv[1], int(sys.argv[2])
os.makedirs(os.path.dirname(out), exist_ok=True)
for spec in sys.argv[3:]:
    name, cmd = spec.split("=", 1)
    for rep in range(reps):
        for arm in ("parent", "new"):
            t0 = time.time()
            p = subprocess.run(["timeout", "-k", "10", "240"] + cmd.split(), cwd=REPO, capture_output=True, text=True,
                               env=dict(os.environ, MAGENT_LIB=LIBS[arm]))
            if p.returncode != 0:
                print("FAILED", name, arm, rep, p.returncode, p.stdout[-2000:], p.stderr[-3000:], flush=True)
                sys.exit(1)
            lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
            with open(out, "a") as fh:
                for ln in lines:
                    fh.write(json.dumps({"bench": name, "lib": arm, "lib_sha256_16": SHA[arm], "rep": rep, "result": ln}) + "\n")
            print(name, arm, rep, "%.1fs" % (time.time() - t0), json.dumps(lines)[:300], flush=True)
