"""Device-side helpers of the merge matcher's GPU tests: upload a mergematch_ref scene, run MergeMatcher, download."""
import numpy as np

PAIR_DT = np.dtype([("i", np.int32), ("j", np.int32), ("epi", np.float64), ("ncc", np.float64)])


def upload_cams(cams, device=0):
    """mergematch_ref cameras -> (the dicts MergeMatcher.run takes, the tensors that back them)"""
    import torch

    dev = torch.device("cuda", device)
    out, keep = [], []
    for c in cams:
        xy = torch.as_tensor(np.ascontiguousarray(c["xy"], dtype=np.float64).reshape(-1), device=dev)
        st = torch.as_tensor(np.ascontiguousarray(c["state"], dtype=np.int32), device=dev)
        im = torch.as_tensor(np.ascontiguousarray(c["imgSmall"], dtype=np.uint8), device=dev)
        keep += [xy, st, im]
        out.append(dict(xy=xy.data_ptr(), state=st.data_ptr(), imgSmall=im.data_ptr(), K=np.asarray(c["K"], dtype=np.float64), imgScale=c["imgScale"]))
    return out, keep


def pair_records(cands):
    """[(i, j, epi, ncc)] or [(i, j, ncc)] -> cs_ncc_pair records"""
    a = np.zeros(len(cands), PAIR_DT)
    for q, c in enumerate(cands):
        a[q] = (c[0], c[1], c[2] if len(c) == 4 else 0.0, c[-1])
    return a


def from_pairs(mm, lists, xy1, xy2, seeds=None, max_disp=150.0, counts=None, device=0):
    """run cs_merge_match_from_pairs_dev on candidate lists (one per job; positions shared) -> [(matches [n][2], scores [n], count row)]"""
    import torch

    dev = torch.device("cuda", device)
    keep, dp, dc = [], [], []
    for q, cands in enumerate(lists):
        rec = pair_records(cands)
        t = torch.as_tensor(np.frombuffer(rec.tobytes() + b"\0" * 24, np.uint8).copy(), device=dev)
        n = torch.as_tensor(np.array([len(rec) if counts is None else counts[q]], np.int32), device=dev)
        keep += [t, n]
        dp.append(t.data_ptr()), dc.append(n.data_ptr())
    a = torch.as_tensor(np.ascontiguousarray(xy1, dtype=np.float64).reshape(-1), device=dev)
    b = torch.as_tensor(np.ascontiguousarray(xy2, dtype=np.float64).reshape(-1), device=dev)
    mm.from_pairs(dp, dc, [a.data_ptr()] * len(lists), [b.data_ptr()] * len(lists), seeds, max_disp)
    cnt = mm.counts(len(lists))
    del keep
    return [(*mm.matches(k, cnt[k][0]), cnt[k]) for k in range(len(lists))]


def as_arrays(matches):
    """[(i, j, score)] -> (int32 [n][2], float64 [n])"""
    m = np.array([(c[0], c[1]) for c in matches], np.int32).reshape(-1, 2)
    return m, np.array([c[2] for c in matches], np.float64)
