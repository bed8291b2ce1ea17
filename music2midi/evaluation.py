from music2midi_amd.evaluation import (evaluate_batch, evaluate_tokens,  # noqa: F401
                                       extract_midi_melody, melody_chroma_accuracy, note_scores_tokens)
