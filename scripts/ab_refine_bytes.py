"""Byte-for-byte A/B of the corpus path between two builds of the library: runs a fixed matrix of `Corpus` calls with
whichever library OSC_LIB_PATH names (this tree's build when unset) and writes one sha256 per output array as JSON.  Run it
once per library, each in a fresh process, and compare the files; `--compare A B` does that and exits non-zero unless every
digest is equal.

The matrix: seed 7, N = 4096, D in {96, 384, 768, 1024, 1280, 1536} (1, 2, 3, 4 and -- twice -- 6 columns per thread of
k_cq_solve / k_cq_settle), Q = 40 under OSC_CORPUS_CHUNK=16 (a ragged last chunk), top_k in {1, 50, 100}, gates in {None,
"diffusion", a given array, all ones}, receipts in {None, "light", "full"}, all with as_arrays=True; the dict form for one
configuration; and search, diffusion_gates_many (direct and cg) and _candidate_graph.

    OSC_LIB_PATH=/path/to/parent/liboscillink_hip.so python scripts/ab_refine_bytes.py --out parent.json
    python scripts/ab_refine_bytes.py --out new.json
    python scripts/ab_refine_bytes.py --compare parent.json new.json"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, Q, SEED = 4096, 40, 7
DS = (96, 384, 768, 1024, 1280, 1536)
TOP_KS = (1, 50, 100)
RECEIPTS = (None, "light", "full")


def digest(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def compare(pa: str, pb: str) -> int:
    with open(pa) as f:
        a = json.load(f)["digests"]
    with open(pb) as f:
        b = json.load(f)["digests"]
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(json.dumps({"a": pa, "b": pb, "digests": len(a), "differing": len(diff), "first": diff[:10]}))
    return 1 if diff or len(a) != len(b) else 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_refine_bytes.json"))
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    os.environ["OSC_CORPUS_CHUNK"] = "16"  # read when a Corpus is created
    from oscillink_amd import Corpus, _native as nat

    out = {}

    def put(key, arrays):
        for name, v in arrays.items():
            out[f"{key}/{name}"] = digest(v)

    for D in DS:
        rng = np.random.default_rng(SEED + D)
        centers = rng.standard_normal((8, D)).astype(np.float32) * 2
        Y = (centers[rng.integers(0, 8, N)] + 0.5 * rng.standard_normal((N, D))).astype(np.float32)
        P = (Y[rng.integers(0, N, Q)] + 0.5 * rng.standard_normal((Q, D))).astype(np.float32)
        with Corpus(Y) as c:
            for top_k in TOP_KS:
                given = rng.uniform(0.0, 1.5, (Q, top_k)).astype(np.float32)
                gates = {"none": None, "diffusion": "diffusion", "given": given, "ones": np.ones((Q, top_k), np.float32)}
                for gname, g in gates.items():
                    for rec in RECEIPTS:
                        put(f"D{D}/K{top_k}/gates={gname}/receipts={rec}",
                            c.refine_many(P, top_k, 8, as_arrays=True, gates=g, gate_gamma=0.15, receipts=rec))
                ids, cos = c.search(P, top_k)
                put(f"D{D}/K{top_k}/search", {"ids": ids, "cos": cos})
                for method in ("direct", "cg"):
                    put(f"D{D}/K{top_k}/diffusion_gates_many/{method}",
                        c.diffusion_gates_many(P, top_k, gamma=0.15, method=method))
                put(f"D{D}/K{top_k}/candidate_graph",
                    dict(zip(("rowptr", "col", "a", "w", "sqrt_deg"), c._candidate_graph(P[3], top_k))))
            if D == 768:  # the dict form: every value of it, through its canonical JSON
                for gname, g in (("none", None), ("diffusion", "diffusion")):
                    r = c.refine_many(P, 100, 8, gates=g, gate_gamma=0.15, receipts="full")
                    out[f"D{D}/K100/gates={gname}/receipts=full/dicts"] = hashlib.sha256(
                        json.dumps(r, sort_keys=True).encode()).hexdigest()
                out[f"D{D}/K100/gates=none/receipts=None/dicts"] = hashlib.sha256(
                    json.dumps(c.refine_many(P, 100, 8), sort_keys=True).encode()).hexdigest()
    rec = {"N": N, "Q": Q, "seed": SEED, "D": list(DS), "top_k": list(TOP_KS), "chunk": 16,
           "library": "OSC_LIB_PATH" if os.environ.get("OSC_LIB_PATH") else "this tree", "digests": out}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(json.dumps({"out": a.out, "digests": len(out), "library": nat.LIB_PATH}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
