"""Cost of a Bermudan chain entry (omc_chain_entry::exercise_every) against the American entry.

1M paths x 252 steps, put at K = 100: GBM on folded storage and Heston (full truncation) on full storage.  Per
configuration, in ONE process, alternating, medians of `reps` after `warm` warm-ups of the chain's HIP-event phase times
(omc_chain_info: ms_pass1 = pass-1 sweeps + reductions, ms_pass2 = table builds + pass-2 sweeps + finalizes) of the
one-entry chains
    american (exercise_every = 0)       every = 5, 21, 63
and, with --parent-lib FILE (a libomc.so built from the parent commit, loaded beside this tree's in the same process),
    the parent's American one-entry chain, and omc_price_american -- the headline pricing -- on both libraries.
The expectation is read from the code, not measured: a sweep is bound per row it visits, a Bermudan entry's sweeps visit
(N - 1) / k + 1 of the N rows, so their time should fall towards that share of the American entry's, down to the
latency-bound small launches that every entry keeps (about 46 us).  Each line reports, per schedule,
the measured share and the share of rows.
One JSON line per configuration, on stdout and appended to --out FILE (the committed record: profiles/bermudan_time.txt).
Every configuration runs in a child process of its own under a time limit; the first that fails ends the run.
usage: time_bermudan.py [--parent-lib FILE] [--out FILE] [reps] [warm]"""
import ctypes as C
import json
import os
import statistics as st
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = ["gbm", "heston"]
M, N = 1_000_000, 252
SCHEDULES = (5, 21, 63)
LIMIT_S = 300


def context_on(libpath):
    """A Context of the binding on another build of the library (same ABI number, hence the same signatures)."""
    from options_model_amd import _ffi
    lib = C.CDLL(libpath)
    for name, (res, args) in _ffi.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    assert lib.omc_abi_version() == _ffi.ABI_VERSION
    c = object.__new__(_ffi.Context)
    h = C.c_void_p()
    _ffi._check(lib, lib.omc_ctx_create(0, None, C.byref(h)))
    c.lib, c.handle, c.device, c._arrays, c._hook = lib, h, 0, set(), None
    return c


def one(model, reps, warm, parent_lib, out_file):
    sys.path.insert(0, ROOT)
    from options_model_amd import _ffi
    ctx = _ffi.default_context(0)
    kw = dict(model="heston", heston_scheme="full_truncation") if model == "heston" else {}
    p = _ffi.make_params(semantics="two_pass", is_put=True, n_paths=M, n_steps=N, K=100.0, seed=42, **kw)

    def chain(c, every):
        outs, info = c.price_american_chain(p, [100.0], True, exercise_every=every)
        return dict(pass1=info["ms_pass1"], pass2=info["ms_pass2"], total=info["ms_total"], paths=info["ms_paths"],
                    price=outs[0]["price"], folded=info["folded"])

    def single(c):
        o = c.price_american(p)
        return dict(pass1=o["ms_pass1"], pass2=o["ms_pass2"], total=o["ms_total"], paths=o["ms_paths"], price=o["price"],
                    folded=o["folded"])

    runs = {"american": lambda: chain(ctx, 0)}
    for k in SCHEDULES:
        runs[f"every_{k}"] = lambda k=k: chain(ctx, k)
    runs["headline"] = lambda: single(ctx)
    if parent_lib:
        pctx = context_on(parent_lib)
        runs["parent_american"] = lambda: chain(pctx, 0)     # (the parent reads no schedule: the word is its reserved one)
        runs["parent_headline"] = lambda: single(pctx)
    samples = {k: [] for k in runs}
    for it in range(warm + reps):
        for k, fn in runs.items():  # alternating: every variant sees the same state of the machine
            r = fn()
            if it >= warm:
                samples[k].append(r)
    out = dict(model=model, M=M, N=N, reps=reps, warm=warm)
    for k, rs in samples.items():
        out[k] = {f: st.median(r[f] for r in rs) for f in rs[0]}
        out[k]["min_pass1"], out[k]["max_pass1"] = min(r["pass1"] for r in rs), max(r["pass1"] for r in rs)
        out[k]["min_pass2"], out[k]["max_pass2"] = min(r["pass2"] for r in rs), max(r["pass2"] for r in rs)
    am = out["american"]
    for k in SCHEDULES:
        e = out[f"every_{k}"]
        e["rows_share"] = ((N - 1) // k + 1) / N
        e["pass1_share"], e["pass2_share"] = e["pass1"] / am["pass1"], e["pass2"] / am["pass2"]
    assert out["american"]["price"] == out["headline"]["price"]
    if parent_lib:
        assert out["parent_american"]["price"] == am["price"] and out["parent_headline"]["price"] == am["price"]
    print(json.dumps(out), flush=True)
    if out_file:
        with open(out_file, "a") as f:
            f.write(json.dumps(out) + "\n")


def main(argv):
    opts = {}
    for flag in ("--out", "--parent-lib"):
        if flag in argv:
            i = argv.index(flag)
            opts[flag] = os.path.abspath(argv[i + 1])
            argv = argv[:i] + argv[i + 2:]
    if argv and argv[0] == "--one":
        return one(argv[1], int(argv[2]), int(argv[3]), opts.get("--parent-lib"), opts.get("--out"))
    nums = [int(v) for v in argv if not v.startswith("--")]
    reps, warm = (nums + [9, 3])[:2] if len(nums) < 2 else nums[:2]
    for model in CONFIGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--one", model, str(reps), str(warm)]
        for flag, v in opts.items():
            cmd += [flag, v]
        try:
            rc = subprocess.run(cmd, timeout=LIMIT_S).returncode
        except subprocess.TimeoutExpired:
            print(f"time_bermudan: {model} ran out of time ({LIMIT_S} s); nothing more is started", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"time_bermudan: {model} ended with status {rc}; nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
