"""Components of the kept edges at config 4 (`simulate_graph(50000, 20, 0.2, 100, 20)`, N = 1e6, E = 7.47e7):

  * the three launches of pangnn_components_i32 (init, hook, compress) by events, median after warm-up, for
    keep = y as int32 and as bool (the true groups), keep = the thresholded logits of a freshly initialised model (int32,
    as predict_homolog_genes returns them), and keep = None;
  * the whole homolog_groups call (the launches, the status read, the torch compaction), wall time;
  * the host's scipy.sparse.csgraph.connected_components on the same kept edges (edges already on the host: the
    device-to-host copy of edge_index and keep is timed apart), and that the labels agree.

Each kernel figure is set against the hook pass's algorithmic bytes E * keep_itemsize + kept * 16 + N * (4 + 1) (16 B per
edge without keep) and the arithmetic bound at 8 TB/s.

    python tools/time_components.py --out profiles/components.jsonl
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/time_components.py --kernel-only      # a run of its own

On a shared machine run each GPU step under its own time limit, e.g. `timeout -k 10 600 python tools/time_components.py`.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BPS = 8e12


def _median_ms(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def _wall_ms(fn, steps):
    import torch
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="graph, then the kernel calls only (for rocprofv3)")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy comparison")
    ap.add_argument("--out", default=None, help="append the JSON lines here")
    a = ap.parse_args()

    import torch
    import pangnn_amd
    from pangnn_amd import _lib, postprocessing, simulate
    dev = torch.device("cuda")
    lib = _lib.load()
    g = simulate.simulate_graph(50000, 20, 0.2, 100, 20, seed=0, device=dev)
    n, e = g.num_nodes, g.edge_index.shape[1]
    ei = g.edge_index.contiguous()
    torch.manual_seed(0)
    model = pangnn_amd.AlternateGCN(dev, None, False, dims=[64, 128], num_nodes=n)
    model.eval()
    with torch.no_grad():
        logits = model(g).detach().reshape(-1).float()
    model_pred = (torch.sigmoid(logits) >= 0.72).int()                    # predict_homolog_genes' default threshold
    del model, logits
    y_i32 = (g.y > 0.5).int()
    cases = [("y_int32", y_i32), ("y_bool", y_i32.bool()), ("fresh_model_int32", model_pred), ("none", None)]
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    touched = torch.empty(n, dtype=torch.uint8, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)

    for name, keep in cases:
        def call():
            _lib.check(lib.pangnn_components_i32(ei[0].data_ptr(), ei[1].data_ptr(), _lib.ptr(keep),
                                                 0 if keep is None else keep.element_size(), e, n, labels.data_ptr(),
                                                 touched.data_ptr(), status.data_ptr(), _lib.stream_ptr()),
                       "pangnn_components_i32")
        med, mn = _median_ms(call, a.steps, a.warmup)
        kept = e if keep is None else int((keep != 0).sum())
        item = 0 if keep is None else keep.element_size()
        nbytes = e * item + kept * 16 + n * (4 + 1)
        comps = int((labels.long() == torch.arange(n, device=dev)).sum())
        emit(dict(what="three_launches", keep=name, E=e, N=n, kept=kept, kept_fraction=kept / e, ms=med, ms_min=mn,
                  hook_algorithmic_bytes=nbytes, achieved_TBps=nbytes / med / 1e9, bound_ms_at_8TBps=nbytes / HBM_BPS * 1e3,
                  components=comps, touched=int(touched.sum()), status=int(status.item())))
    torch.cuda.synchronize()
    if a.kernel_only:
        return

    for name, keep in cases[:3]:
        med, mn = _wall_ms(lambda: postprocessing.homolog_groups(ei, keep, n), max(a.steps // 4, 3))
        grp = postprocessing.homolog_groups(ei, keep, n)
        emit(dict(what="homolog_groups", keep=name, wall_ms=med, wall_ms_min=mn, groups=grp.num_groups,
                  members=int(grp.members.numel())))
    true = postprocessing.homolog_groups(ei, y_i32, n)
    pred = postprocessing.homolog_groups(ei, model_pred, n)
    med, mn = _wall_ms(lambda: postprocessing.group_agreement(pred, true), 3)
    emit(dict(what="group_agreement", pred="fresh_model_int32", true="y", wall_ms=med, **postprocessing.group_agreement(pred, true)))

    if not a.no_host:
        import numpy as np
        import scipy.sparse as sp
        from scipy.sparse.csgraph import connected_components as scipy_components
        for name, keep in cases[:3]:
            t0 = time.perf_counter()
            h_ei, h_keep = ei.cpu().numpy(), keep.cpu().numpy()
            copy_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            on = h_keep != 0
            s, d = h_ei[0][on], h_ei[1][on]
            m = sp.coo_matrix((np.ones(s.size, dtype=np.int8), (s, d)), shape=(n, n))
            _, comp = scipy_components(m, directed=False)
            smallest = np.full(comp.max() + 1, n, dtype=np.int64)
            np.minimum.at(smallest, comp, np.arange(n))
            host_ms = (time.perf_counter() - t0) * 1e3
            got = postprocessing.connected_components(ei, keep, n)[0].cpu().numpy()
            emit(dict(what="host_scipy", keep=name, copy_to_host_ms=copy_ms, select_build_components_min_ms=host_ms,
                      labels_equal=bool((got == smallest[comp]).all())))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
