"""CPU tests of the row-sharded products (enlsip_gn_tsqr_products*): the derived allowance of tests/tsqr_product_cases.py is
certified on a NumPy restatement of the kernels' chunked order (inside on every case) and on two mutations of it (outside on every
case), and the Python stage driver enlsip_gn.tsqr.tsqr_products is run over gloo with two ranks and a NumPy local stage."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import tsqr_product_cases as pc

CASES = [(name, n, with_p) for name in pc.splits() for n in pc.NS for with_p in (False, True)]
_REFS = {}


def _case(name, n, with_p):
    key = (name, n, with_p)
    if key not in _REFS:
        heights = pc.splits()[name]
        J, rx, p = pc.problem(pc.case_seed(name, n, with_p), sum(heights), n, with_p)
        _REFS[key] = (J, rx, p, heights, pc.Reference(J, rx, p, len(heights)))
    return _REFS[key]


def test_constants_and_message_length_match_the_library():
    import __graft_entry__ as ge
    ge.build()
    import enlsip_gn._lib as L
    from enlsip_gn.tsqr import tsqr_products_msg_len, PRODUCTS_HDR
    lib = L.load()
    assert pc.chunk_height() % 64 == 0 and PRODUCTS_HDR == pc.header_doubles()
    for n in (1, 2, 5, 64, 65, 1024):
        want = pc.msg_len(n)
        assert want % 2 == 0 and want >= pc.header_doubles() + n + 3
        assert lib.enlsip_gn_tsqr_products_msg_len(n) == want == tsqr_products_msg_len(n)
    assert lib.enlsip_gn_tsqr_products_msg_len(0) == 0


@pytest.mark.parametrize("name,n,with_p", CASES)
def test_chunked_order_stays_inside_the_allowance(name, n, with_p):
    J, rx, p, heights, ref = _case(name, n, with_p)
    grad, sums = pc.chunked_products(J, rx, p, heights, pc.chunk_height())
    assert ref.check(grad, sums, name) is None
    if p is None:
        assert sums[1] == 0.0 and sums[2] == 0.0


@pytest.mark.parametrize("name,n,with_p", CASES)
def test_a_dropped_row_and_a_skipped_chunk_leave_the_allowance(name, n, with_p):
    """The allowance is tight enough to see ONE row of one shard, or one chunk's partial, missing"""
    J, rx, p, heights, ref = _case(name, n, with_p)
    g = max(range(len(heights)), key=lambda i: (heights[i] > 0, i))      # the last shard that has rows
    grad, sums = pc.chunked_products(J, rx, p, heights, pc.chunk_height(), drop_last_row_of=g)
    assert ref.check(grad, sums, name) is not None
    grad, sums = pc.chunked_products(J, rx, p, heights, pc.chunk_height(), skip_chunk_of=g)
    assert ref.check(grad, sums, name) is not None


def test_host_combine_adds_in_rank_order_and_checks_the_headers():
    from enlsip_gn.tsqr import products_combine_host, tsqr_products_msg_len, PRODUCTS_HDR as H
    n, G = 5, 3
    L = tsqr_products_msg_len(n)
    rng = np.random.default_rng(5)
    M = np.zeros((G, L))
    M[:, H:H + n + 3] = rng.standard_normal((G, n + 3)) * 10.0 ** rng.integers(-8, 8, (G, n + 3))
    M[:, 0], M[:, 1], M[:, 2] = np.arange(1, G + 1), G, n
    grad, sums = products_combine_host(M.ravel(), G, n)
    want = (M[0, H:H + n + 3] + M[1, H:H + n + 3]) + M[2, H:H + n + 3]
    assert np.array_equal(np.concatenate([grad, sums]), want)
    for col, val in ((2, n + 1), (1, G + 1), (0, 3)):
        B = M.copy()
        B[1, col] = val
        with pytest.raises(ValueError):
            products_combine_host(B.ravel(), G, n)
    B = M.copy()
    B[:, 0] = 0.0
    B[:, 1] = 0.0                                    # "not stated" passes
    assert np.array_equal(products_combine_host(B.ravel(), G, n)[0], grad)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, m, n, with_p, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from enlsip_gn.tsqr import tsqr_products, row_range
    J, rx, p = pc.problem(88, m, n, with_p)
    lo, hi = row_range(m, world, rank)
    J_loc = torch.from_numpy(np.ascontiguousarray(J[lo:hi].T))
    rx_loc = torch.from_numpy(rx[lo:hi].copy())
    res = tsqr_products(None, J_loc, rx_loc, p, local_stage=pc.np_local_stage)
    np.savez(out + f".{rank}.npz", grad=res.grad, sums=res.sums, Jp=np.zeros(0) if res.Jp is None else res.Jp.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("m,n,with_p", [(pc.chunk_height() + 131, 5, True), (300, 65, False)])
def test_products_driver_gloo_world2(tmp_path, m, n, with_p):
    port = _free_port()
    out = str(tmp_path / "res")
    mp.spawn(_worker, args=(2, port, m, n, with_p, out), nprocs=2, join=True)
    from enlsip_gn.tsqr import row_range
    J, rx, p = pc.problem(88, m, n, with_p)
    ref = pc.Reference(J, rx, p, 2)
    r0, r1 = np.load(out + ".0.npz"), np.load(out + ".1.npz")
    for r in (r0, r1):
        assert ref.check(r["grad"], r["sums"], f"m={m} n={n}") is None
    assert np.array_equal(r0["grad"].view(np.uint64), r1["grad"].view(np.uint64))       # every rank holds the same bits
    assert np.array_equal(r0["sums"].view(np.uint64), r1["sums"].view(np.uint64))
    if with_p:
        Jp = np.concatenate([r0["Jp"], r1["Jp"]])
        assert Jp.shape == (m,) and np.all(np.abs(Jp - ref.Jp) <= ref.Jp_bound)
        assert r0["Jp"].shape == (row_range(m, 2, 0)[1],)
