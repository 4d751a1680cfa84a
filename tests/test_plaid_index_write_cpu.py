"""CPU: write_plaid_index writes the index directory the reference's indexer writes (third_party/ColBERT/colbert/indexing/
index_saver.py:79-90, collection_indexer.py:366-449) and read_plaid_index reads back: the file set, dtypes and shapes, the chunk
metadata, metadata.json, ivf.pid.pt through the writer save_ivf uses, passage_ids.json, and the refusals.  Pure host code: torch and
json, no device."""
import json
import os

import pytest
import torch

D, NBITS, C, RB = 64, 2, 8, 16
CHUNK_PASSAGES = (5, 5, 2)


def _codec(cutoffs=True):
    from rmr_amd import PlaidCodec
    gen = torch.Generator().manual_seed(5)
    cen = torch.nn.functional.normalize(torch.randn(C, D, generator=gen), dim=-1)
    w = torch.tensor([-0.2, -0.05, 0.05, 0.2])
    codec = PlaidCodec(cen, w, NBITS, bucket_cutoffs=torch.tensor([-0.1, 0.0, 0.1]) if cutoffs else None)
    codec.avg_residual = 0.125
    return codec


def _chunks(seed=9):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for n in CHUNK_PASSAGES:
        doclens = torch.randint(1, 9, (n,), generator=gen).tolist()
        R = sum(doclens)
        out.append((torch.randint(0, C, (R,), generator=gen, dtype=torch.int32), torch.randint(0, 256, (R, RB), generator=gen, dtype=torch.uint8),
                    doclens))
    return out


def _load(path):
    return torch.load(path, map_location="cpu", weights_only=True)


def test_the_directory_holds_what_the_indexer_writes_and_reads_back(tmp_path):
    from rmr_amd import read_plaid_index, write_plaid_index
    codec, chunks, d = _codec(), _chunks(), str(tmp_path / "index")
    assert codec.residual_bytes == RB
    meta = write_plaid_index(d, codec, iter(chunks), config={"query_maxlen": 32})
    want = {"centroids.pt", "buckets.pt", "avg_residual.pt", "metadata.json"}
    for i in range(3):
        want |= {f"{i}.codes.pt", f"{i}.residuals.pt", f"doclens.{i}.json", f"{i}.metadata.json"}
    assert set(os.listdir(d)) == want, "no ivf.pid.pt, no passage_ids.json and no plan.json unless asked for"
    passages = embeddings = 0
    for i, (codes, res, doclens) in enumerate(chunks):
        got_c, got_r = _load(os.path.join(d, f"{i}.codes.pt")), _load(os.path.join(d, f"{i}.residuals.pt"))
        assert got_c.dtype == torch.int32 and tuple(got_c.shape) == (sum(doclens),) and torch.equal(got_c, codes)
        assert got_r.dtype == torch.uint8 and tuple(got_r.shape) == (sum(doclens), RB) and torch.equal(got_r, res)
        with open(os.path.join(d, f"doclens.{i}.json")) as f:
            got_d = json.load(f)
        assert got_d == doclens and all(type(x) is int for x in got_d)
        with open(os.path.join(d, f"{i}.metadata.json")) as f:
            assert json.load(f) == {"passage_offset": passages, "num_passages": len(doclens), "num_embeddings": sum(doclens),
                                    "embedding_offset": embeddings}
        passages, embeddings = passages + len(doclens), embeddings + sum(doclens)
    assert passages == 12
    with open(os.path.join(d, "metadata.json")) as f:
        on_disk = json.load(f)
    assert on_disk == meta and set(meta) == {"config", "num_chunks", "num_partitions", "num_embeddings", "avg_doclen"}
    assert meta["config"] == {"dim": D, "nbits": NBITS, "query_maxlen": 32}
    assert (meta["num_chunks"], meta["num_partitions"], meta["num_embeddings"]) == (3, C, embeddings)
    assert meta["avg_doclen"] == embeddings / 12
    assert float(_load(os.path.join(d, "avg_residual.pt"))) == 0.125
    back, got = read_plaid_index(d)
    assert back.nbits == NBITS and torch.equal(back.centroids, codec.centroids) and torch.equal(back.bucket_weights, codec.bucket_weights)
    assert torch.equal(back.bucket_cutoffs, codec.bucket_cutoffs)
    got = list(got)
    assert len(got) == 3
    first = 0
    for (f0, codes, res, doclens), (wc, wr, wd) in zip(got, chunks):
        assert f0 == first and torch.equal(codes, wc) and torch.equal(res, wr) and doclens == wd
        first += len(wd)


def test_the_inverted_file_goes_through_the_writer_of_save_ivf(tmp_path):
    from rmr_amd import write_ivf, write_plaid_index
    pids = torch.tensor([0, 3, 11, 2, 5, 0, 1, 2, 3, 4], dtype=torch.int32)
    lengths = torch.tensor([3, 0, 2, 5, 0, 0, 0, 0], dtype=torch.int64)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    write_plaid_index(a, _codec(), iter(_chunks()), ivf=(pids, lengths))
    assert write_ivf(b, (pids, lengths)) == os.path.join(b, "ivf.pid.pt")
    with open(os.path.join(a, "ivf.pid.pt"), "rb") as f, open(os.path.join(b, "ivf.pid.pt"), "rb") as g:
        assert f.read() == g.read(), "the bytes of the file"
    got_pids, got_lengths = _load(os.path.join(a, "ivf.pid.pt"))
    assert got_pids.dtype == torch.int32 and got_lengths.dtype == torch.int64
    assert torch.equal(got_pids, pids) and torch.equal(got_lengths, lengths)
    with pytest.raises(ValueError):
        write_ivf(b, (pids[:-1], lengths))


def test_passage_ids_are_written_only_where_json_keeps_them(tmp_path):
    from rmr_amd import write_plaid_index
    ids = [f"doc{i}" if i % 2 else i for i in range(12)]
    d = str(tmp_path / "ids")
    write_plaid_index(d, _codec(), iter(_chunks()), passage_ids=ids)
    with open(os.path.join(d, "passage_ids.json")) as f:
        assert json.load(f) == ids
    for j, bad in enumerate(((1, 2), 1.5, None, True)):
        d = str(tmp_path / f"no_ids{j}")
        write_plaid_index(d, _codec(), iter(_chunks()), passage_ids=ids[:-1] + [bad])
        assert "passage_ids.json" not in os.listdir(d) and "metadata.json" in os.listdir(d)
    with pytest.raises(ValueError, match="11 passage ids for 12"):
        write_plaid_index(str(tmp_path / "short"), _codec(), iter(_chunks()), passage_ids=ids[:-1])


def test_refusals(tmp_path):
    from rmr_amd import write_plaid_index
    chunks = _chunks()
    d = str(tmp_path / "no_cutoffs")
    with pytest.raises(ValueError, match="bucket_cutoffs"):
        write_plaid_index(d, _codec(cutoffs=False), iter(chunks))
    assert not os.path.exists(d), "a codec without cutoffs is refused before anything is written"
    codes, res, doclens = chunks[1]
    with pytest.raises(ValueError, match="chunk 1"):
        write_plaid_index(str(tmp_path / "sum"), _codec(), iter([chunks[0], (codes, res, doclens[:-1] + [doclens[-1] + 1]), chunks[2]]))
    with pytest.raises(ValueError, match="chunk 1"):
        write_plaid_index(str(tmp_path / "zero"), _codec(), iter([chunks[0], (codes, res, doclens + [0]), chunks[2]]))
    with pytest.raises(ValueError, match=r"chunk 0: residuals must be uint8 \[\d+, 16\]"):
        write_plaid_index(str(tmp_path / "width"), _codec(), iter([(chunks[0][0], chunks[0][1][:, :8], chunks[0][2])]))
    with pytest.raises(ValueError, match="no chunk"):
        write_plaid_index(str(tmp_path / "none"), _codec(), iter([]))
