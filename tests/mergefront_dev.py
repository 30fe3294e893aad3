"""Device-side helpers of the merge front's GPU tests: upload mergefront_scenes cameras, run MergeFront, download a job's layers."""
import numpy as np


def upload_cams(cams, device=0):
    """cameras dict(pts [n][2], desc [n][dim], K) -> (the dicts MergeFront takes, the tensors that back them)"""
    import torch

    dev = torch.device("cuda", device)
    out, keep = [], []
    for c in cams:
        p = torch.as_tensor(np.ascontiguousarray(c["pts"], dtype=np.float64).reshape(-1), device=dev)
        d = torch.as_tensor(np.ascontiguousarray(c["desc"], dtype=np.float32).reshape(-1), device=dev)
        keep += [p, d]
        out.append(dict(pts=p.data_ptr() if p.numel() else 0, desc=d.data_ptr() if d.numel() else 0, n=len(c["pts"]),
                        K=np.asarray(c["K"], dtype=np.float64)))
    return out, keep


def filler(dim, K):
    """a camera no job names"""
    return dict(pts=np.zeros((1, 2)), desc=np.zeros((1, dim), np.float32), K=K)


def layers(mf, slot, job, n_hyp, res):
    """everything the device left for one job (at batch slot `slot` of the last batch) -> dict"""
    n = res["surf_num"]
    m, d = mf.matches(job, n)
    smp, cnt, E = mf.hypotheses(slot, n_hyp)
    return dict(res, matches=m, dist=d, inlier=mf.inlier_flags(job, n).astype(bool), seeds=mf.seeds(job, res["inlier_num"]),
                new_matches=mf.new_matches(job, res["inlier_num"]), hyp_sample=smp, hyp_count=cnt, hyp_E=E, pix=mf.point_rows(slot, n))
