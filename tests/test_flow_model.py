"""tests/flow_model.py pinned to the C oracle (oracle/txflow.c) on the inputs the GPU edge tests use:
B1's power vectors (totals up to tendermint's MaxTotalVotingPower) over its 140-vote stream with
replays, flipped and second signatures, nil votes and bad addresses, and A1's key family (prefixes,
zero tails, keys equal up to one byte).  Statuses, fired bits, query and the set count are equal, so
what tests/test_flow_edges.py expects of the kernels is two independent restatements that agree.
The oracle verifies every signature itself; the model is handed the verdict the test built."""
import pytest

import flow_model as M

CHAIN = b"test_chain_id"


def _keys(n):
    import oracle as O
    return M.validator_keys(O, n)


def _compare(oracle_lib, pubs, addrs, powers, votes, verdicts, cut, keys):
    flow = oracle_lib.Flow(pubs, powers, CHAIN)
    model = M.FlowModel(addrs, powers)
    n_ev = 0
    for s in range(0, len(votes), cut):
        part, ok = votes[s:s + cut], verdicts[s:s + cut]
        ost, osum, ofired = flow.add_votes(part)
        st, fired, events = model.add_votes(part, ok)
        assert st == [int(x) for x in ost], f"statuses differ in the batch at {s}"
        assert fired == [bool(x) for x in ofired], f"fired bits differ in the batch at {s}"
        for e in events:                     # the crossing vote is a fired ADDED vote; the oracle's running sum agrees
            assert ofired[e["vote_index"]] and int(osum[e["vote_index"]]) >= model.quorum
        n_ev += len(events)
    for k in keys:
        assert model.query(k) == flow.query(k)
        assert model.get_votes(k) == flow.get_votes(k)
    assert model.num_sets() == flow.num_sets()
    return model, n_ev


@pytest.mark.parametrize("which", range(len(M.B1_POWERS)))
def test_model_matches_oracle_b1_powers(oracle_lib, which):
    powers = M.B1_POWERS[which]
    assert all(p >= 0 for p in powers) and sum(powers) <= M.MAXT
    seeds, pubs, addrs = _keys(M.B1_VALS)
    hashes = M.b1_hashes()
    assert len(set(hashes)) == M.B1_TXS and all(len(h) == 64 for h in hashes)
    signer = M.Signer(oracle_lib, seeds, addrs, CHAIN)
    votes, ok = signer.votes([(hashes[t], v, kind) for t, v, kind in M.b1_stream()])
    model, n_ev = _compare(oracle_lib, pubs, addrs, powers, votes, ok, M.B1_CUT, hashes)
    assert n_ev == M.B1_TXS                  # every tx gets all seven validators: each one commits
    assert all(model.query(h) == (sum(powers), True) for h in hashes)


def test_b1_stream_reaches_every_status(oracle_lib):
    seeds, pubs, addrs = _keys(M.B1_VALS)
    hashes = M.b1_hashes()
    votes, ok = M.Signer(oracle_lib, seeds, addrs, CHAIN).votes([(hashes[t], v, k) for t, v, k in M.b1_stream()])
    st = M.FlowModel(addrs, M.B1_POWERS[0]).add_votes(votes, ok)[0]
    assert set(st) == set(range(7))


def test_model_matches_oracle_key_family(oracle_lib):
    keys = M.key_family()
    assert len(keys) >= 320 and len(set(keys)) == len(keys)
    seeds, pubs, addrs = _keys(4)
    signer = M.Signer(oracle_lib, seeds, addrs, CHAIN)
    votes, ok = signer.votes([(keys[k], v, "ok") for k, v in M.family_order(len(keys))])
    model, n_ev = _compare(oracle_lib, pubs, addrs, [1, 1, 1, 1], votes, ok, 300, keys)
    assert model.quorum == 3 and n_ev == len(keys) == model.num_sets()
    assert all(model.query(k) == (3, True) for k in keys)
