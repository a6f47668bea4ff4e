"""Inputs the GPU tests of the merge family (test_merge_gpu.py, test_ties_gpu.py, test_dare_gpu.py, test_pairstats_gpu.py,
test_band_gpu.py, test_della_gpu.py, test_tall_gpu.py, test_emr_gpu.py) share."""
import functools

import numpy as np
import torch

from oracle import synth
from oracle.detweights import det_array


def base_size_state():
    """(experts, central) as numpy dicts: the base-size all_moe block tensors and the ufo central checkpoint (salt 7) -- the inputs
    tests/golden/merge_base_digests.json pins."""
    sd = {k: det_array(k, s) for k, (s, dt) in synth.block_shapes(768, 3072, "all_moe").items()}
    central = {k: det_array(k, s, 7) for k, (s, dt) in synth.block_shapes(768, 3072, "ufo").items()}
    return sd, central


TINY_LENGTHS = [5, 1, 4097, 3, 2, 4099]


def tiny_job_shapes(n_cus):
    """(length, sources) of 2 x 12 x n_cus + 7 jobs: more chunks than twice the widest grid of the family (12 workgroups per CU),
    so every workgroup's run of chunks holds several jobs.  Lengths cycle through TINY_LENGTHS, sources through 1 .. 4."""
    return [(TINY_LENGTHS[i % len(TINY_LENGTHS)], 1 + i % 4) for i in range(2 * 12 * n_cus + 7)]


@functools.lru_cache(maxsize=1)
def tiny_jobs(n_cus, planted):
    """[(central, sources)] for tiny_job_shapes(n_cus), built once: `planted` (test_ties_gpu.py) data, which has two sources at
    least; a third and fourth are the central tensor plus noise.  Read-only for its users."""
    rng = np.random.default_rng(8)
    jobs = []
    for i, (n, S) in enumerate(tiny_job_shapes(n_cus)):
        c, srcs = planted(n, max(S, 2), seed=1000 + i)
        while len(srcs) < S:
            srcs.append((c + rng.standard_normal(n).astype(np.float32) * np.float32(0.3)).astype(np.float32))
        jobs.append((c, srcs[:S]))
    return jobs


def one_buffer(arrays):
    """Copies fp32 arrays into ONE device buffer, each at a 16-byte aligned offset; returns their views, in order."""
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.size + 3) // 4 * 4
    host = np.zeros(total, np.float32)
    for a, o in zip(arrays, offs):
        host[o:o + a.size] = a.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 16 == 0
    return [buf[o:o + a.size] for a, o in zip(arrays, offs)]


# ---------------------------------------------------------------- the plans with packed masks (test_tall_gpu.py, test_emr_gpu.py)
def dev_words(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def words_of(t):
    return t.cpu().numpy().view("<u4")


def poison(plan, outs):
    """Outputs start as NaN and mask outputs as all ones: every float and every word that survives a run was written by it."""
    for o in outs:
        o.fill_(float("nan"))
    for job, ms in zip(plan.jobs, plan.masks):
        if ms is not None and job.op == 0:
            for m in ms:
                m.fill_(-1)
