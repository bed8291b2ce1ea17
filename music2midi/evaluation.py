from music2midi_amd.evaluation import (evaluate_batch, evaluate_midi_result, evaluate_tokens,  # noqa: F401
                                       extract_midi_melody, frame_scores_tokens, melody_chroma_accuracy, note_scores_tokens)
