"""Host side of the steerable lifting kernels (csrc/steer_lift.hip): the packed weight layout against the layout its file header
documents, and the shape predicate and size getters through the built library.  No GPU."""
import pytest
import torch

from equiadapt_amd import _lib, ops

CASES = [(1, 5, 1), (3, 7, 4), (3, 7, 16), (3, 9, 5), (1, 9, 16), (3, 5, 64), (1, 7, 3), (3, 5, 2), (1, 5, 7)]


def _unpack(wpk: torch.Tensor, cin: int, k: int, fields: int) -> torch.Tensor:
    """The bank read back from wpk element by element of the documented layout:
    wpk[g][b][s][lane] = w[16 (g bpw + b) + (lane & 15)][ci][ky][kx], ky = s // (rwp / 4), c = 4 (s % (rwp / 4)) + (lane >> 4) = kx cin + ci;
    every other element must be zero."""
    groups, bpw, steps, _ = wpk.shape
    rwp = (k * cin + 3) // 4 * 4
    c9 = 9 * fields
    bank = torch.zeros(c9, cin, k, k)
    seen = torch.zeros_like(bank, dtype=torch.bool)
    for g in range(groups):
        for b in range(bpw):
            for s in range(steps):
                for lane in range(64):
                    co = 16 * (g * bpw + b) + (lane & 15)
                    ky, c = s // (rwp // 4), 4 * (s % (rwp // 4)) + (lane >> 4)
                    v = float(wpk[g, b, s, lane])
                    if co < c9 and c < k * cin:
                        bank[co, c % cin, ky, c // cin] = v
                        seen[co, c % cin, ky, c // cin] = True
                    else:
                        assert v == 0.0, (g, b, s, lane)
    assert seen.all()
    return bank


@pytest.mark.parametrize("cin,k,fields", CASES)
def test_pack_round_trip(cin, k, fields):
    lib = _lib.load()
    bank = torch.randn(9 * fields, cin, k, k, generator=torch.Generator().manual_seed(fields))
    wpk = ops.pack_steer_lift_weights(bank)
    groups, bpw, steps, rwp = ops.steer_lift_layout(cin, k, fields)
    nblk = (9 * fields + 15) // 16
    assert wpk.shape == (groups, bpw, steps, 64) and wpk.dtype == torch.float32 and wpk.is_contiguous()
    assert bpw <= 3 and groups * bpw >= nblk and (groups - 1) * bpw < nblk          # whole blocks, no empty group
    assert steps == k * rwp // 4 and rwp % 4 == 0 and 0 <= rwp - k * cin < 4
    assert wpk.numel() == lib.eqa_steer_lift_packed_floats(cin, k, fields)
    assert torch.equal(_unpack(wpk, cin, k, fields), bank)
    # a channels-last bank (what the network caches) packs to the same operand
    assert torch.equal(ops.pack_steer_lift_weights(bank.contiguous(memory_format=torch.channels_last)), wpk)


def test_supported_predicate_and_getters():
    lib = _lib.load()
    F = lib.eqa_field_norm_max_fields()
    for cin in range(0, 5):
        for k in range(1, 13):
            for fields in (0, 1, 2, 16, F, F + 1):
                want = cin in (1, 3) and k in (5, 7, 9) and 1 <= fields <= F
                assert bool(lib.eqa_steer_lift_supported(cin, k, fields)) == want == ops.steer_lift_supported(cin, k, fields)
                assert (lib.eqa_steer_lift_packed_floats(cin, k, fields) > 0) == want
                assert (lib.eqa_steer_lift_wgrad_workspace_bytes(cin, k, fields) > 0) == want
    assert all(lib.eqa_steer_lift_supported(3, 7, f) for f in range(1, F + 1))      # every field count, 9 F rarely a multiple of 16
    assert lib.eqa_steer_lift_stat_rows(0) < 0 and lib.eqa_steer_lift_stat_rows(F + 1) < 0
    for fields in range(1, F + 1):
        groups, bpw, _, _ = ops.steer_lift_layout(3, 7, fields)
        assert lib.eqa_steer_lift_stat_rows(fields) == 1024 // groups
        assert lib.eqa_steer_lift_wgrad_workspace_bytes(3, 7, fields) == (1024 // groups) * groups * 16 * bpw * 160 * 4


def test_wrappers_refuse_cpu_tensors():
    bank = torch.randn(36, 3, 7, 7)
    wpk = ops.pack_steer_lift_weights(bank)
    x = torch.randn(1, 3, 9, 9).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError):
        ops.steer_lift(x, wpk, 7, 4)
    with pytest.raises(RuntimeError):
        ops.steer_lift_wgrad(x, torch.randn(1, 36, 3, 3).contiguous(memory_format=torch.channels_last), 7)
    with pytest.raises(ValueError):
        ops.pack_steer_lift_weights(torch.randn(35, 3, 7, 7))
