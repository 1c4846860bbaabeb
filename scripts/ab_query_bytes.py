"""Byte-for-byte A/B of the batched lattice calls (osc_query.hip's nine drivers) between two checkouts: runs a fixed matrix
of `Oscillink` calls with the package and library of `--tree` (this tree when not given; built already) and writes one sha256
per output array as JSON.  Run it once per checkout, each in a fresh process, and compare the files; `--compare A B` does
that and exits non-zero unless every digest is equal.

The matrix: seed 7, lattices (N, D, kneighbors) = (700, 40, 6) and (1500, 72, 8) -- a padded GEMM K and 2 and 3 gate slabs
per query -- each under OSC_REORDER=0 and 1 on a fresh handle, after a settle (U != Y); every call with as_arrays=True.
  plain, Q = 300 (chunks of 256 + 44): bundle_many(k=8), _mmr_many, receipt_many light and full, the latter with
      OSCILLINK_RECEIPT_NULL_CAP unset, 16 and (N = 1500) 1100, which is above the device selection's limit;
  chain receipts, Q = 300: one shared 5-node chain and per-query chains of 2 to 9 nodes, again on the lattice's own weighted
      chain (add_chain);
  chain priors, Q = 40: chain_receipt_many, bundle_many and receipt_many (light, full) with chains, weights given and None,
      lamP 0 and 0.2, and with OSC_CHAIN_PRIOR_COLS=16, under which the call takes several passes (the count, replayed from
      the packer's rule, is printed);
  gated, Q = 40 under OSC_GATED_CHUNK=16 (16 + 16 + 8): diffusion_gates_many (direct, cg), bundle_gated_many (given gates,
      "diffusion"), _ustar_gated_many, receipt_gated_many over settle x detail x bundle_k.
Timing arrays (`*_ms`) are left out; everything else the calls return, and the per-query reports in `last_*`, is digested.

    python scripts/ab_query_bytes.py --tree /path/to/parent/checkout --out parent.json
    python scripts/ab_query_bytes.py --out this.json
    python scripts/ab_query_bytes.py --compare parent.json this.json

A full record holds about 1 900 digests.  `--brief FULL OUT` rolls them up into one sha256 (and array count) per lattice,
row order and call family -- the form kept under profiles/; `--compare` takes either form."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 7
LATTICES = ((700, 40, 6), (1500, 72, 8))
Q_PLAIN, Q_SMALL = 300, 40
PRIOR_COLS, GATED_CHUNK = 16, 16
NULL_CAP = "OSCILLINK_RECEIPT_NULL_CAP"


def digest(a) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def rollup(digests: dict) -> dict:
    """One sha256 per (lattice, row order, call family) over that group's `key=digest` lines in key order, with the count."""
    groups = {}
    for k in sorted(digests):
        groups.setdefault("/".join(k.split("/")[:3]), []).append(f"{k}={digests[k]}\n")
    return {g: f"{len(v)}:{hashlib.sha256(''.join(v).encode()).hexdigest()}" for g, v in groups.items()}


def brief(src: str, dst: str) -> int:
    """The record of `src` with its per-array digests replaced by their rollup: the form small enough to keep in git."""
    with open(src) as f:
        rec = json.load(f)
    rec["arrays"] = len(rec["digests"])
    rec["digests"] = rollup(rec.pop("digests"))
    with open(dst, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    return 0


def compare(pa: str, pb: str) -> int:
    with open(pa) as f:
        a = json.load(f)["digests"]
    with open(pb) as f:
        b = json.load(f)["digests"]
    diff = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print(json.dumps({"a": pa, "b": pb, "digests": len(a), "differing": len(diff), "first": diff[:10]}))
    return 1 if diff or len(a) != len(b) else 0


def prior_passes(chains, max_cols: int) -> int:
    """The passes of a chain-prior call whose only binding limit is `max_cols` distinct nodes a pass (the packer's rule)."""
    passes, cols = 0, set()
    for ch in chains:
        d = set(int(c) for c in ch)
        if not cols or len(cols | d) > max_cols:
            passes, cols = passes + 1, set()
        cols |= d
    return passes


def run_lattice(Oscillink, N, D, kn, reorder, put, notes):
    os.environ["OSC_REORDER"] = str(reorder)  # read when the handle is created
    rng = np.random.default_rng(SEED + N)
    centers = rng.standard_normal((8, D)).astype(np.float32) * 2
    Y = (centers[rng.integers(0, 8, N)] + 0.5 * rng.standard_normal((N, D))).astype(np.float32)
    P = (Y[rng.integers(0, N, Q_PLAIN)] + 0.5 * rng.standard_normal((Q_PLAIN, D))).astype(np.float32)
    scores = rng.standard_normal((N, Q_PLAIN)).astype(np.float32)
    shared = [int(c) for c in rng.choice(N, 5, replace=False)]
    chains = [[int(c) for c in rng.choice(N, 2 + q % 8, replace=False)] for q in range(Q_PLAIN)]
    weights = [[0.5 + 0.125 * ((q + t) % 9) for t in range(len(chains[q]) - 1)] for q in range(Q_SMALL)]
    own = [int(c) for c in rng.choice(N, 6, replace=False)]
    tag = f"N{N}/reorder{reorder}"
    lat = Oscillink(Y, kneighbors=kn, deterministic_k=True)
    try:
        lat.set_query(P[0])
        lat.settle()

        def receipts(key, psis, caps, **kw):
            for detail in ("light", "full"):
                lat.set_receipt_detail(detail)
                for cap in caps if detail == "full" else (None,):
                    if cap is not None:
                        os.environ[NULL_CAP] = str(cap)
                    put(f"{key}/receipt_many/{detail}/cap={cap}", lat.receipt_many(psis, as_arrays=True, **kw))
                    os.environ.pop(NULL_CAP, None)

        # plain
        put(f"{tag}/bundle_many", lat.bundle_many(P, 8, as_arrays=True))
        put(f"{tag}/mmr_many", lat._mmr_many(scores, 8, 0.5))
        receipts(tag, P, (None, 16) + ((1100,) if N == 1500 else ()))

        # chain receipts
        def chain_receipts(key):
            put(f"{key}/chain_receipt_many/shared", lat.chain_receipt_many(P, shared, as_arrays=True))
            put(f"{key}/chain_receipt_many/per_query", lat.chain_receipt_many(P, chains, as_arrays=True))

        chain_receipts(tag)
        # chain priors
        Ps, cs = P[:Q_SMALL], chains[:Q_SMALL]

        def priors(key, lamP, w):
            kw = dict(chains=cs, lamP=lamP, chain_weights=w)
            put(f"{key}/chain_receipt_many", lat.chain_receipt_many(Ps, cs, lamP=lamP, chain_weights=w, as_arrays=True))
            put(f"{key}/bundle_many", lat.bundle_many(Ps, 8, as_arrays=True, **kw))
            put(f"{key}/bundle_many/last", lat.last_bundle_prior)
            receipts(key, Ps, (None,), **kw)
            put(f"{key}/receipt_many/last", lat.last_receipt_prior)

        for lamP in (0.0, 0.2):
            for wname, w in (("given", weights), ("none", None)):
                priors(f"{tag}/prior/lamP={lamP}/weights={wname}", lamP, w)
        os.environ["OSC_CHAIN_PRIOR_COLS"] = str(PRIOR_COLS)
        priors(f"{tag}/prior/cols={PRIOR_COLS}", 0.2, weights)
        del os.environ["OSC_CHAIN_PRIOR_COLS"]
        notes[f"{tag}/prior/cols={PRIOR_COLS}/passes"] = prior_passes(cs, PRIOR_COLS)
        # gated
        os.environ["OSC_GATED_CHUNK"] = str(GATED_CHUNK)
        for method in ("direct", "cg"):
            put(f"{tag}/diffusion_gates_many/{method}", lat.diffusion_gates_many(Ps, gamma=0.15, method=method))
        G = lat.diffusion_gates_many(Ps, gamma=0.15)["gates"]
        for gname, g in (("given", G), ("diffusion", "diffusion")):
            put(f"{tag}/bundle_gated_many/{gname}", lat.bundle_gated_many(Ps, g, 8, as_arrays=True, gate_gamma=0.15))
            put(f"{tag}/bundle_gated_many/{gname}/last", lat.last_bundle_gated)
        put(f"{tag}/ustar_gated_many", lat._ustar_gated_many(Ps, G))
        for detail in ("light", "full"):
            lat.set_receipt_detail(detail)
            for settle in (None, True):
                for bk in (None, 8):
                    key = f"{tag}/receipt_gated_many/{detail}/settle={settle}/bundle_k={bk}"
                    put(key, lat.receipt_gated_many(Ps, G, settle=settle, bundle_k=bk, as_arrays=True))
                    put(f"{key}/last", lat.last_receipt_gated)
        put(f"{tag}/receipt_gated_many/diffusion",
            lat.receipt_gated_many(Ps, "diffusion", settle=True, bundle_k=8, as_arrays=True, gate_gamma=0.15))
        del os.environ["OSC_GATED_CHUNK"]
        # the lattice's own weighted chain
        lat.add_chain(own, 0.2, weights=[0.5, 1.0, 1.5, 0.75, 1.25])
        chain_receipts(f"{tag}/own_chain")
    finally:
        lat.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab_query_bytes.json"))
    ap.add_argument("--tree", default=ROOT, help="the checkout to import oscillink_amd from (built already)")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--brief", nargs=2, metavar=("FULL", "OUT"), help="roll a full record up per call family")
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if a.brief:
        return brief(*a.brief)
    sys.path.insert(0, os.path.abspath(a.tree))
    for name in (NULL_CAP, "OSC_CHAIN_PRIOR_COLS", "OSC_GATED_CHUNK", "OSCILLINK_RECEIPT_DYNAMICS"):
        os.environ.pop(name, None)
    from oscillink_amd import Oscillink, _native as nat

    out, notes = {}, {}

    def put(key, value):
        if isinstance(value, np.ndarray):
            value = {"array": value}
        elif isinstance(value, tuple):
            value = {str(i): v for i, v in enumerate(value)}
        for name, v in value.items():
            if isinstance(v, np.ndarray) and not name.endswith("_ms"):
                out[f"{key}/{name}"] = digest(v)

    for N, D, kn in LATTICES:
        for reorder in (0, 1):
            run_lattice(Oscillink, N, D, kn, reorder, put, notes)
    rec = {"seed": SEED, "lattices": [list(x) for x in LATTICES], "Q": [Q_PLAIN, Q_SMALL], "gated_chunk": GATED_CHUNK,
           "prior_cols": PRIOR_COLS, "notes": notes, "digests": out}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(json.dumps({"out": a.out, "digests": len(out), "library": nat.LIB_PATH, **notes}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
