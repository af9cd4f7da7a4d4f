#!/usr/bin/env python3
"""Generate max-candidate labelling fixtures from the reference's OWN baseline code.

TEST INFRASTRUCTURE ONLY.  Runs in the build container (needs the reference tree, which never travels to the GPU box);
the `candidates_<cfg>.npz` files it writes under tests/golden/ are the only thing the test-suite reads.

What is pinned: the three "best hit per genome" labelings of predict_homolog_genes (src/predict.py:83-90),
  * src/helper.py:437-485 calculate_baseline_labels  (Q-score and raw-score labels, as dataset.py:390 calls it on the whole
    graph: sim_score_dict = Q-scores, sim_score_dict_raw = raw scores after trivial-case removal, self hits included);
  * src/helper.py:494-546 init_worker + find_max_logit (the logit labels of calculate_logit_baseline_labels, called serially
    on one chunk instead of through its multiprocessing.Pool).
The logits fed to find_max_logit are seeded normals quantised to 1/8 (many exact ties), with planted tied maxima, one NaN,
some +inf and some -inf.

How: the stub / subprocess / PYTHONHASHSEED=0 technique of make_fixtures.py (which this imports and leaves as it is): the
dataset is rebuilt exactly as that script builds it, then the labels are mapped onto the existing fixture's
`whole_edge_index` by their (src, dst) key.

Output per config: labels_q, labels_raw, labels_logit (uint8) and logits (float32), all in the order of
`<cfg>.npz:whole_edge_index`.

Usage:  python tests/golden/make_candidate_fixtures.py            # all configs
        python tests/golden/make_candidate_fixtures.py --only sim_200x4
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_fixtures import CONFIGS, REF, STUB   # noqa: E402


def seeded_logits(edge_index, genome_of, seed):
    """float32 logits in the order of edge_index: N(0, 2) quantised to 1/8, every 5th multi-edge segment's maximum tied,
    +inf / -inf on a few edges, one NaN"""
    import numpy as np
    rng = np.random.default_rng(seed)
    e = edge_index.shape[1]
    v = (np.round(rng.normal(0.0, 2.0, e) * 8.0) / 8.0).astype(np.float32)
    src, dst = edge_index
    g = int(genome_of.max()) + 1
    key = src * g + genome_of[dst]
    order = np.argsort(key, kind="stable")
    ks = key[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    ends = np.r_[starts[1:], e]
    for k, (b, t) in enumerate(zip(starts, ends)):
        if t - b >= 2 and k % 5 == 0:
            members = order[b:t]
            m = members[np.argmax(v[members])]
            other = members[members != m][0]
            v[other] = v[m]                             # two maxima
    pick = rng.permutation(e)
    v[pick[:3]] = np.inf
    v[pick[3:6]] = -np.inf
    v[pick[6]] = np.nan
    return v


def child(name, out_path):
    """Runs inside the per-config subprocess (cwd = scratch dir, stub dir + reference on sys.path)."""
    import random
    import numpy as np
    import torch
    random.seed(0); np.random.seed(0); torch.manual_seed(0)

    import src.setup as setup            # parses sys.argv (setup.py:53)
    import src.dataset as ds
    import src.helper as helper

    class SerialPool:                    # dataset.py:140 uses Pool(...).map
        def __init__(self, *a, **k): pass
        def __enter__(self): return self
        def __exit__(self, *a): return False
        def map(self, fn, it): return [fn(x) for x in it]
    ds.Pool = SerialPool

    args = setup.args
    if args.simulate_dataset:
        dset = ds.UnionGraphDataset(calculate_baseline=True, split=(0.7, 0.15, 0.01), categorical_nodes=False)
    else:
        dset = ds.UnionGraphDataset(args.annotation, args.similarity, args.ribap_groups, split=(0.7, 0.15, 0.01),
                                    categorical_nodes=False, calculate_baseline=True)
    whole = dset.generate_graphs()
    genes = list(dset.gene_str_ids_lst)
    pos = dset.gene_id_position_dict

    fix = np.load(os.path.join(HERE, f"{name}.npz"))
    fix_ei = fix["whole_edge_index"]
    genome_of = fix["genome_of"].astype(np.int64)
    n = int(fix["num_nodes"])
    ref_src, ref_dst = (x.tolist() for x in whole.edge_index)
    ref_key = np.array(ref_src, dtype=np.int64) * n + np.array(ref_dst, dtype=np.int64)
    fix_key = fix_ei[0] * n + fix_ei[1]
    assert np.array_equal(np.sort(ref_key), np.sort(fix_key)), "the rebuilt graph is not the fixture's"
    to_ref = {k: i for i, k in enumerate(ref_key.tolist())}
    at = np.array([to_ref[k] for k in fix_key.tolist()], dtype=np.int64)   # fixture position -> reference position

    # Q-score and raw-score labels, as dataset.py:390 computes them for the whole graph
    lq, lraw = helper.calculate_baseline_labels(whole.edge_index, genes, dset.sim_score_dict, dset.sim_score_dict_raw)

    # logit labels: seeded logits in fixture order, handed to the reference in its own edge order
    logits = seeded_logits(fix_ei, genome_of, seed=sum(map(ord, name)))
    ref_logits = np.empty_like(logits)
    ref_logits[at] = logits
    ref_logits = [float(x) for x in ref_logits]
    logit_dict = {(s, t): ref_logits[i] for i, (s, t) in enumerate(zip(ref_src, ref_dst))}
    helper.init_worker(ref_src, genes, dset.sim_score_dict, pos, logit_dict)
    ll = helper.find_max_logit(ref_src, ref_dst, ref_logits)

    out = dict(
        labels_q=np.asarray(lq, dtype=np.uint8)[at],
        labels_raw=np.asarray(lraw, dtype=np.uint8)[at],
        labels_logit=np.asarray(ll, dtype=np.uint8)[at],
        logits=logits,
    )
    np.savez_compressed(out_path, **out)
    print(json.dumps({"config": name, "E": int(fix_key.size), "q": int(out["labels_q"].sum()),
                      "raw": int(out["labels_raw"].sum()), "logit": int(out["labels_logit"].sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--out", default=None)
    a, rest = ap.parse_known_args()
    if a.child:
        sys.argv = ["pangnn.py"] + rest
        child(a.child, a.out)
        return
    if not os.path.isdir(REF):
        sys.exit("needs the reference tree (build container only)")
    with tempfile.TemporaryDirectory(prefix="pangnn_cand_") as tmp:
        stub_dir = os.path.join(tmp, "stubs")
        for rel, body in STUB.items():
            p = os.path.join(stub_dir, rel)
            os.makedirs(os.path.dirname(p), exist_ok=True)
            with open(p, "w") as f:
                f.write(body)
        for name, (argv, _) in CONFIGS.items():
            if a.only and a.only != name:
                continue
            work = os.path.join(tmp, name)
            os.makedirs(work)
            env = dict(os.environ, PYTHONHASHSEED="0", PYTHONPATH=f"{stub_dir}:{REF}", MPLBACKEND="Agg", COLUMNS="200")
            out_path = os.path.join(HERE, f"candidates_{name}.npz")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--out", out_path] + argv
            r = subprocess.run(cmd, cwd=work, env=env, capture_output=True, text=True)
            tail = [l for l in r.stdout.splitlines() if l.startswith("{")]
            print(name, "rc=", r.returncode, tail[-1] if tail else r.stderr[-3000:])


if __name__ == "__main__":
    main()
