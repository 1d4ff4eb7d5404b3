"""Which route TiledStepper takes (geonomics_amd/parallel.py), without a device: stub shard,
stub comm, use_library=False so that nothing joins the library's communicator.  `v2` is the
Python-driven device protocol (tile2), `dev_transport` says the payloads stay in device memory;
with neither, the step goes through the host-staged protocol."""
import pytest

from geonomics_amd.parallel import TiledStepper

W = H = 64          # 2 x 2 tiles of 32 x 32: wider than 3 hash cells at mating radius 1


class _Shard:
    """what the oracle shard looks like to the constructor: no `.dev`"""
    n_traits, W64 = 0, 1

    def tile_set(self, R, C, r, c):
        self.tile = (R, C, r, c)


class _HipShard(_Shard):
    dev = object()


class _Comm:
    rank, dist = 0, None

    def __init__(self, world, device):
        self.world, self.device = world, device


CASES = {
    # name: (shard, world, comm device, mating radius, GNX_TILE_TRANSPORT) -> (dev_transport, v2)
    'hip_world1': ((_HipShard, 1, 'cpu', 1.0, None), (False, True)),
    'hip_world4_cuda': ((_HipShard, 4, 'cuda', 1.0, None), (True, True)),
    'hip_world4_cpu': ((_HipShard, 4, 'cpu', 1.0, None), (False, False)),
    'panmixia': ((_HipShard, 4, 'cuda', None, None), (False, False)),
    'transport_host': ((_HipShard, 4, 'cuda', 1.0, 'host'), (False, False)),
    'oracle_shard_world1': ((_Shard, 1, 'cpu', 1.0, None), (False, False)),
    'oracle_shard_world4': ((_Shard, 4, 'cuda', 1.0, None), (False, False)),
}


def _stepper(monkeypatch, shard, world, device, radius, transport):
    monkeypatch.delenv('GNX_TILE_TRANSPORT', raising=False)
    if transport is not None:
        monkeypatch.setenv('GNX_TILE_TRANSPORT', transport)
    st = TiledStepper(shard(), _Comm(world, device), W, H, radius, use_library=False)
    assert st.v3 is False
    return st


@pytest.mark.parametrize('name', sorted(CASES))
def test_route_choice(monkeypatch, name):
    monkeypatch.delenv('GNX_TILE_V2', raising=False)
    args, (dev_transport, v2) = CASES[name]
    st = _stepper(monkeypatch, *args)
    assert (bool(st.dev_transport), bool(st.v2)) == (dev_transport, v2)


@pytest.mark.parametrize('name', sorted(CASES))
def test_retired_switch_changes_nothing(monkeypatch, name):
    """GNX_TILE_V2=0 once sent a device-capable transport through a staged protocol with device
    payloads; that protocol is gone and the variable is not read"""
    monkeypatch.setenv('GNX_TILE_V2', '0')
    args, (dev_transport, v2) = CASES[name]
    st = _stepper(monkeypatch, *args)
    assert (bool(st.dev_transport), bool(st.v2)) == (dev_transport, v2)
