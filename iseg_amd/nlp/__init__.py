"""nlp/ of the reference: text models that can drive a text-conditioned head."""
