"""Training callbacks of the reference recipe (reference deadtrees/callbacks/), driven by ``trainer.fit(callbacks=)``."""
