"""Index factory and small helpers with the reference's names
(backend/utils.py:29-41, 222-232, 293-330)."""
from __future__ import annotations

from . import faiss_compat as faiss
from .config import Config

config = Config()


def chunkIt(seq, num):
    """Divide a sequence into roughly equal parts (backend/utils.py:29-41)."""
    avg = len(seq) / float(num)
    out = []
    last = 0.0
    while last < len(seq):
        out.append(seq[int(last): int(last + avg)])
        last += avg
    return out


def get_images_paths():
    """rglob over EXTENSIONS under DATA_FOLDER_PATH (backend/utils.py:222-232)."""
    paths = []
    for ext in config.EXTENSIONS:
        paths.extend(config.DATA_FOLDER_PATH.rglob(ext))
    return paths


def get_image(image_path):
    """Thumbnail of an image as base64 JPEG (PNG if JPEG cannot encode it), None if the
    file is missing (backend/utils.py:44-62).  Display only."""
    import base64
    import io

    from PIL import Image

    size = config.THUMBNAIL_SIZE, config.THUMBNAIL_SIZE
    try:
        img = Image.open(image_path, mode="r")
    except FileNotFoundError:
        return None
    img.thumbnail(size, Image.LANCZOS)
    buf = io.BytesIO()
    try:
        img.save(buf, format="JPEG")
    except OSError:
        img.save(buf, format="PNG")
    return base64.encodebytes(buf.getvalue()).decode("ascii")


def hamming(a, b):
    """Hamming distance between two integer hashes (the signature of backend/utils.py:84-88, which nothing in the
    reference calls)."""
    return (int(a) ^ int(b)).bit_count()


def hashes_to_codes(hashes, nbits=64):
    """Python-int hashes, as the reference's ``dhash`` yields them (bit i has the value 2**i, backend/utils.py:65-76),
    as the uint8 (n, nbits / 8) codes of ``faiss.IndexBinaryFlat(nbits)``: little-endian, bit i of a hash is bit
    ``i % 8`` of byte ``i // 8``.  The index's distance between ``codes[a]`` and ``codes[b]`` is then
    ``hamming(hashes[a], hashes[b])``."""
    import numpy as np

    nbits = int(nbits)
    assert nbits > 0 and nbits % 8 == 0, "nbits must be a positive multiple of 8"
    hashes = [int(h) for h in hashes]
    out = np.zeros((len(hashes), nbits // 8), dtype=np.uint8)
    for i, h in enumerate(hashes):
        assert 0 <= h < (1 << nbits), f"hash {h} does not fit in {nbits} bits"
        out[i] = np.frombuffer(h.to_bytes(nbits // 8, "little"), dtype=np.uint8)
    return out


def create_search_index(data_array, index_type="cosine"):
    """backend/utils.py:293-330.  'cosine' -> IndexFlatIP over rows normalised IN
    PLACE in the caller's array (quirk 5.9-6); 'l2' -> IndexFlatL2; then add.
    'cell-probe' is IndexIVFPQ with Faiss's default residual codes, which is not provided (NotImplementedError before any
    device call); 'cell-probe-pq' is that branch (backend/utils.py:311-325) with by_residual=False: IndexIVFPQ over an L2
    coarse quantiser with the reference's 8 centroids, m = 16 codes of 8 bits and nprobe = 5, trained on the data, then
    add.  'cell-probe-flat' is that branch
    (backend/utils.py:311-325) without the product quantiser: IndexIVFFlat over an L2 coarse quantiser with the
    reference's 8 centroids and nprobe = 5, trained on the data, then add.  'pq' is that branch's product quantiser
    without the lists: IndexPQ with the reference's m = 16 codes of 8 bits, trained on the data, then add.
    'pq-refine' is that index under IndexRefineFlat: its k * 16 best rows re-ranked by their exact float32 distance.
    'sq8' is IndexScalarQuantizer with QT_8bit: one byte per entry between the data's per-dimension minimum and maximum,
    trained on the data, then add.  'cell-probe-sq8' is the cell-probe branch with that quantiser in place of the product
    quantiser: IndexIVFScalarQuantizer (QT_8bit, by_residual=False) over an L2 coarse quantiser with the reference's 8
    centroids and nprobe = 5, trained on the data, then add.  'pca256-l2' is the textbook reduction of a long descriptor:
    IndexPreTransform(PCAMatrix(d, min(256, d)), IndexFlatL2), trained on the data, then add.  'opq-pq' is the 'pq' index
    behind an OPQ rotation: IndexPreTransform(OPQMatrix(d, 16), IndexPQ(d, 16, 8)), trained on the data, then add."""
    num_features = data_array.shape[1]
    if index_type == "cosine":
        index = faiss.IndexFlatIP(num_features)
        faiss.normalize_L2(data_array)
    elif index_type == "l2":
        index = faiss.IndexFlatL2(num_features)
    elif index_type == "cell-probe":
        raise NotImplementedError("'cell-probe' is IndexIVFPQ with Faiss's default by_residual = True, which is not "
                                  "provided: 'cell-probe-pq' is the same index over codes of the rows themselves")
    elif index_type == "cell-probe-flat":
        ncentroids = 8
        coarse_quantizer = faiss.IndexFlatL2(num_features)
        index = faiss.IndexIVFFlat(coarse_quantizer, num_features, ncentroids)
        index.nprobe = 5  # find n most similar clusters
        index.train(data_array)
    elif index_type == "pq":
        m = 16  # number of bytes per vector
        index = faiss.IndexPQ(num_features, m, 8)
        index.train(data_array)
    elif index_type == "pq-refine":
        index = faiss.IndexRefineFlat(faiss.IndexPQ(num_features, 16, 8))
        # a choice, not a tuned value: the reference's k = 20 then asks the product quantiser for 320 candidates
        index.k_factor = 16
        index.train(data_array)
    elif index_type == "sq8":
        index = faiss.IndexScalarQuantizer(num_features, faiss.ScalarQuantizer.QT_8bit)
        index.train(data_array)
    elif index_type == "cell-probe-pq":
        ncentroids = 8
        code_size = 16
        coarse_quantizer = faiss.IndexFlatL2(num_features)
        index = faiss.IndexIVFPQ(coarse_quantizer, num_features, ncentroids, code_size, 8, by_residual=False)
        index.nprobe = 5  # find n most similar clusters
        index.train(data_array)
    elif index_type == "cell-probe-sq8":
        ncentroids = 8
        coarse_quantizer = faiss.IndexFlatL2(num_features)
        index = faiss.IndexIVFScalarQuantizer(coarse_quantizer, num_features, ncentroids, faiss.ScalarQuantizer.QT_8bit,
                                              faiss.METRIC_L2, by_residual=False)
        index.nprobe = 5  # find n most similar clusters
        index.train(data_array)
    elif index_type == "pca256-l2":
        d_out = min(256, num_features)
        index = faiss.IndexPreTransform(faiss.PCAMatrix(num_features, d_out), faiss.IndexFlatL2(d_out))
        index.train(data_array)
    elif index_type == "opq-pq":
        index = faiss.IndexPreTransform(faiss.OPQMatrix(num_features, 16), faiss.IndexPQ(num_features, 16, 8))
        index.train(data_array)
    else:
        raise ValueError(f"unknown index_type {index_type!r}")
    index.add(data_array)
    print(f"There are {index.ntotal} images in the search index.")
    return index
