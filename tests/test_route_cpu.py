"""CPU: the kernel route of an MPN block (route.block_route) pinned for the benchmark shapes and for every switch.

The shape queries are host functions of the library, so no GPU is needed; a stub stands in for a topology (the predicates read a
handful of its attributes).  The batches' ELL widths and tile counts are those ``topology.get_topology`` reports on an MI355X for
``synthetic.make_batch(grids, B, seed=1)``.  The expected routes are what the predicates of ``_ensure_plans`` / ``_mpn_forward`` /
``_mpn_backward`` gave for these inputs BEFORE they moved into ``route.py`` (transcribed and evaluated next to the new function, which
agreed with them on a grid of 40 435 200 points); they are not output of the function under test."""
import inspect
import types

import pytest

from conftest import load_pkg

# name -> (nrb, ntiles, N, ell, ellT, max_nnz, max_nnzT, max_tile_rows); every ELL tile array present, no graph beyond the tiles
BATCHES = {
    "cigre14_4096": (2, 1024, 61440, 3, 3, 192, 192, 60),        # C2: 64-row tiles, four 15-bus graphs each
    "cigre14_64": (2, 16, 960, 3, 3, 192, 192, 60),
    "ober_sub_1024": (3, 1024, 71680, 3, 3, 288, 288, 70),       # C3: 96-row tiles, one 70-bus graph each
    "ober_sub_64": (3, 64, 4480, 3, 3, 288, 288, 70),            # ... below the single-group tile count (768)
    "ober179_1024": (6, 1024, 183296, 3, 3, 576, 576, 179),      # the 179-bus feeder: 192-row tiles
    "mixed_4096": (2, 1024, 61440, 4, 4, 256, 256, 60),          # C5 shard: cigre14 + cigre14_reswitched
    "ober179_64": (6, 64, 11456, 3, 3, 576, 576, 179),           # ... 192-row tiles below the single-group tile count
}

FIELDS = ("glob", "fold", "b16", "f16", "n_chain", "use16", "gw", "head", "edge", "g16",
          "bwd_chain", "bwd_use16", "bwd_head", "bwd_head_wgrad", "bwd_edge", "bwd_join", "bwd_g16", "bwd_defer")

# (tag, batch, (dim_hid, n_gnn_layers, K, dim_out), need_dx, in_stack, switch set to False, expected route in the order of FIELDS)
CASES = [
    ('C2', 'cigre14_4096', (128, 4, 2, 2), False, False, None,
     (False, True, (1, 2, 3), True, 3, True, 128, True, True, (False, False, False, False), True, True, True, True, True, True, (False, False, False, False), (False, False, False, False))),
    ('C3', 'ober_sub_1024', (128, 4, 2, 2), False, False, None,
     (False, True, (1, 2, 3), True, 3, True, 256, False, False, (False, False, False, False), True, True, True, True, False, True, (False, False, False, False), (False, False, False, False))),
    ('feeder179', 'ober179_1024', (128, 4, 2, 2), False, False, None,
     (False, True, (1, 2, 3), True, 3, True, 384, False, False, (False, False, False, False), True, True, True, True, False, True, (False, False, False, False), (False, False, False, False))),
    ('C5 model', 'mixed_4096', (256, 8, 2, 2), False, False, None,
     (False, True, (1, 2, 3, 4, 5, 6, 7), True, 7, True, 256, True, False, (False, False, False, False, False, False, False, False), True, True, True, True, False, True, (False, False, False, False, False, False, False, False), (False, False, False, False, False, False, False, False))),
    ('driver block, ober_sub B=64', 'ober_sub_64', (32, 8, 2, 8), True, True, None,
     (False, True, (1, 2, 3, 4, 5, 6, 7), False, 7, True, 0, False, False, (False, False, False, False, False, False, False, False), True, True, False, False, False, True, (False, False, False, False, False, False, False, False), (False, False, False, False, False, False, False, False))),
    ('driver block, ober_sub B=1024', 'ober_sub_1024', (32, 8, 2, 8), True, True, None,
     (False, True, (1, 2, 3, 4, 5, 6, 7), True, 7, True, 64, False, False, (False, False, False, False, False, False, False, False), True, True, False, False, False, True, (False, False, False, False, False, False, False, False), (False, False, False, False, False, False, False, False))),
    ('SkipMPN need_dx', 'cigre14_4096', (128, 4, 2, 8), True, False, None,
     (False, True, (1, 2, 3), True, 3, True, 128, False, False, (False, False, False, False), True, True, False, False, False, True, (False, False, False, False), (False, False, False, False))),
    ('C2 block in a stack', 'cigre14_4096', (128, 4, 2, 2), True, True, None,
     (False, True, (1, 2, 3), True, 3, True, 128, True, False, (False, False, False, False), True, True, True, True, False, True, (False, False, False, False), (False, False, False, False))),
    ('K=3', 'cigre14_64', (64, 3, 3, 2), False, False, None,
     (False, True, (1, 2), False, 2, True, 0, False, False, (False, False, False), True, True, False, False, False, True, (False, False, False), (False, False, False))),
    ('K=4', 'cigre14_64', (64, 3, 4, 2), False, False, None,
     (True, False, (), False, 0, False, 0, False, False, (False, False, False), False, False, False, False, False, False, (False, False, False), (False, False, False))),
    ('L=1', 'cigre14_4096', (128, 1, 2, 2), False, False, None,
     (False, False, (), False, 0, False, 0, False, False, (False,), False, False, False, False, False, False, (False,), (False,))),
    ('L=2', 'ober179_1024', (128, 2, 2, 2), False, False, None,
     (False, True, (1,), False, 0, False, 0, False, False, (True, False), False, False, False, False, False, False, (True, False), (False, False))),
    ('C2, CHAIN_LAYERS off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'CHAIN_LAYERS',
     (False, True, (1, 2, 3), False, 0, False, 0, False, False, (False, False, False, False), False, False, False, False, False, False, (False, False, False, False), (False, True, True, False))),
    ('C2, CHAIN_BF16 off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'CHAIN_BF16',
     (False, True, (), False, 3, False, 0, False, False, (False, False, False, False), True, False, False, False, False, True, (False, False, False, False), (False, False, False, False))),
    ('C2, CHAIN_F16 off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'CHAIN_F16',
     (False, True, (1, 2, 3), False, 3, True, 128, True, False, (False, False, False, False), True, True, True, True, False, True, (False, False, False, False), (False, False, False, False))),
    ('C2, CHAIN_GATE_BITS off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'CHAIN_GATE_BITS',
     (False, True, (1, 2, 3), False, 3, True, 0, True, False, (False, False, False, False), True, True, True, True, False, True, (False, False, False, False), (False, False, False, False))),
    ('C2, CHAIN_HEAD off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'CHAIN_HEAD',
     (False, True, (1, 2, 3), True, 3, True, 128, False, False, (False, False, False, False), True, True, False, False, False, True, (False, False, False, False), (False, False, False, False))),
    ('C2, CHAIN_HEAD_FWD off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'CHAIN_HEAD_FWD',
     (False, True, (1, 2, 3), True, 3, True, 128, False, False, (False, False, False, False), True, True, True, True, True, True, (False, False, False, False), (False, False, False, False))),
    ('C2, CHAIN_HEAD_WGRAD off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'CHAIN_HEAD_WGRAD',
     (False, True, (1, 2, 3), True, 3, True, 128, True, True, (False, False, False, False), True, True, True, False, True, True, (False, False, False, False), (False, False, False, False))),
    ('C2, CHAIN_EDGE off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'CHAIN_EDGE',
     (False, True, (1, 2, 3), True, 3, True, 128, True, False, (False, False, False, False), True, True, True, True, False, True, (False, False, False, False), (False, False, False, False))),
    ('C2, EDGE_TILE_KERNELS off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'EDGE_TILE_KERNELS',
     (False, True, (1, 2, 3), True, 3, True, 128, True, False, (False, False, False, False), True, True, True, True, False, True, (False, False, False, False), (False, False, False, False))),
    ('C2, WGRAD_BATCH off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'WGRAD_BATCH',
     (False, True, (1, 2, 3), False, 3, True, 128, True, False, (False, False, False, False), False, False, False, False, False, False, (False, False, False, False), (False, False, False, False))),
    ('C2, FOLD_W2 off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'FOLD_W2',
     (False, False, (1, 2, 3), True, 3, True, 128, True, False, (False, False, False, False), True, True, True, True, False, False, (False, False, False, False), (True, True, True, False))),
    ('C2, WGRAD_JOIN_FOLDED off', 'cigre14_4096', (128, 4, 2, 2), False, False, 'WGRAD_JOIN_FOLDED',
     (False, True, (1, 2, 3), True, 3, True, 128, True, True, (False, False, False, False), True, True, True, True, True, False, (False, False, False, False), (False, True, True, False))),
    # 192-row tiles, ONE column group, fewer tiles than the split-plane chain takes: there is no multi-wave chain of 192 rows, so the block
    # runs layer by layer -- the route of CHAIN_LAYERS = False (the queries without a tile count said "chained"; the launch refused)
    ('feeder179 B=64, H=32', 'ober179_64', (32, 4, 2, 2), False, False, None,
     (False, True, (1, 2, 3), False, 0, False, 0, False, False, (False,) * 4, False, False, False, False, False, False, (False,) * 4, (False, True, True, False))),
    ('driver block, ober179 B=64', 'ober179_64', (32, 8, 2, 8), True, True, None,
     (False, True, (1, 2, 3, 4, 5, 6, 7), False, 0, False, 0, False, False, (False,) * 8, False, False, False, False, False, False, (False,) * 8,
      (False, True, True, True, True, True, True, False))),
]


def _topo(name):
    nrb, ntiles, N, ell, ellT, nnz, nnzT, rows = BATCHES[name]
    return types.SimpleNamespace(nrb=nrb, ntiles=ntiles, N=N, ell=ell, ellT=ellT, max_nnz=nnz, max_nnzT=nnzT, max_tile_rows=rows,
                                 global_only=False, ell_tiles=1, ellT_tiles=1, ell_ent_tiles=1, ellT_ent_tiles=1)


@pytest.mark.parametrize("tag,batch,dims,need_dx,in_stack,switch,expected", CASES, ids=[c[0] for c in CASES])
def test_block_route_of_the_named_shapes(tag, batch, dims, need_dx, in_stack, switch, expected):
    pkg = load_pkg()
    assert pkg.route.BlockRoute._fields == FIELDS
    hid, L, K, nout = dims
    mod = types.SimpleNamespace(dim_hid=hid, n_gnn_layers=L, K=K, dim_out=nout, dim_featn=8, dim_feate=6)
    keep = getattr(pkg.flags, switch) if switch else None
    if switch:
        setattr(pkg.flags, switch, False)
    try:
        got = pkg.route.block_route(mod, _topo(batch), need_dx, in_stack)
    finally:
        if switch:
            setattr(pkg.flags, switch, keep)
    assert dict(zip(FIELDS, got)) == dict(zip(FIELDS, expected))


def test_a_flag_takes_effect_at_the_next_call():
    """Nothing is cached across calls: the same module and topology objects route differently once a flag is flipped."""
    pkg = load_pkg()
    mod = types.SimpleNamespace(dim_hid=128, n_gnn_layers=4, K=2, dim_out=2, dim_featn=8, dim_feate=6)
    topo = _topo("cigre14_4096")
    assert pkg.route.block_route(mod, topo, False, False).n_chain == 3
    keep = pkg.flags.CHAIN_LAYERS
    pkg.flags.CHAIN_LAYERS = False
    try:
        assert pkg.route.block_route(mod, topo, False, False).n_chain == 0
    finally:
        pkg.flags.CHAIN_LAYERS = keep
    assert pkg.route.block_route(mod, topo, False, False).n_chain == 3


def test_the_backward_evaluates_no_predicate_of_its_own():
    """_mpn_backward and its sections follow the route the forward stored: no flag, no shape query (the second evaluation must not
    grow back)."""
    nw = load_pkg().networks
    for fn in (nw._mpn_backward, nw._bwd_chained, nw._bwd_layers, nw._bwd_deferred_wgrads, nw._BlockBackward):
        src = inspect.getsource(fn)
        assert "FL." not in src and "_supported(" not in src and "is_narrow(" not in src, fn.__name__
