"""Images of mixed sizes -> VLAD descriptors as one batched pipeline: the per-image loop of reference
``demo/anyloc_vlad_generate.py:158-186`` (read, normalise, downscale above ``max_img_size``, crop to multiples of the patch,
extract, VLAD) with every stage batched over the whole set -- device ingest into one buffer
(``preprocess.images_to_input_ragged``), the ragged ViT forward (``DinoV2ExtractFeatures.extract_ragged``) and one VLAD
launch over the packed tokens."""
from . import preprocess


def describe_images(extractor, vlad, images, max_img_size=None):
    """``images``: uint8 [H_i, W_i, 3] arrays / tensors of any sizes; ``extractor``: a ``DinoV2ExtractFeatures``;
    ``vlad``: a fitted ``VLAD``.  -> [n, K*D] VLADs in input order, each what the demo's loop
    (``images_to_input`` -> ``extractor(img)`` -> ``vlad.generate``) gives that image."""
    patch = getattr(getattr(extractor, "dino_model", None), "patch", preprocess.PATCH)     # 14, or 16 for a DINOv3 extractor
    flat, sizes = preprocess.images_to_input_ragged(images, max_img_size, multiple=patch)
    packed = extractor.extract_ragged((flat, sizes), packed=True)
    return vlad.generate_multi(packed)
